"""fp64 reference, rounding floor and cases for the per-node tests of the BevEncode training autograd nodes
(tests/test_train_nodes_gpu.py on the GPU, tests/test_train_nodes_ref_cpu.py for this helper itself).

One unit is  x = cat([x2, bilinear_align_corners(x1, up)]) -> conv (bias-free, weights rounded to bf16 as the kernels
pack them) -> BatchNorm(train) -> (+ residual) -> ReLU,  with the conv stage or the BatchNorm stage optional.

  reference(op, mask)   plain torch in fp64 (F.interpolate, torch.cat, F.conv2d, F.batch_norm, +, ReLU) from the same
                        bf16-rounded operands the node receives; gradients by torch.autograd.grad.  No rounding inside.
                        The ReLU of the BACKWARD is the multiplication by `mask` = [y_kernel > 0] taken from the node's
                        own output (what the kernels do); `mask_check` checks that mask on its own.
  evaluate(op, mask, emulate=True)
                        the same chain written out by hand, with bf16 rounding at the kernels' storage points: the
                        upsampled operand, z, y, dz, the (concatenated) input gradient, the upsample adjoint's output,
                        dres.  Its distance from `reference` is the ROUNDING FLOOR of the case; a kernel may be
                        3 x floor away (fp32 accumulation order, bf16 ties that fall differently), with an absolute
                        minimum of 2^-8 for bf16 outputs and 2e-4 for fp32 outputs.  With emulate=False it is an
                        independent second derivation of the reference (the CPU tests hold the two together), and with
                        `plant=` it is a deliberately wrong reference copy that the bound has to reject.

Errors are measured in two metrics per output: max |a - b| / max |b| and ||a - b|| / ||b||.
"""
import collections

import torch
from torch.nn import functional as F

EPS, MOMENTUM = 1e-5, 0.1
BAND_SCALE = 2.0 ** -7      # band of undecided ReLU elements: |t_ref| <= 2^-7 max |y_ref|
BAND_MAX_FRACTION = 0.05
FACTOR = 3.0
MIN_BF16, MIN_F32 = 2.0 ** -8, 2e-4
BF16_OUTPUTS = ("z", "y", "dz", "dres", "g1", "g2")
F32_OUTPUTS = ("dw", "dgamma", "dbeta", "mean", "invstd", "running_mean", "running_var")

Unit = collections.namedtuple("Unit", "name B H W Cx C2 up Cout res relu need fwd grad")


def U(name, B, H, W, Cx, Cout, C2=0, up=1, res=False, relu=True, need=("x1", "x2", "w", "res"), fwd=None, grad=None):
    return Unit(name, B, H, W, Cx, C2, up, Cout, res, relu, tuple(need), fwd, grad)


# `_ConvBNActFn` over the dispatch table of lss_conv_bn_act_train_fwd / bwd.  fwd / grad: the kernel the forward conv
# and the gradient conv must take (asserted on the GPU with ops.conv_ring_ok / ops.conv_ks_ok before the unit runs).
FUSED = [
    U("up1.conv0_b4", 4, 25, 25, 256, 256, C2=64, up=4, fwd="ring", grad="tile"),
    U("up1.conv3_b4", 4, 100, 100, 256, 256, fwd="ring", grad="ring"),
    U("up2_b4", 4, 100, 100, 256, 128, up=2, fwd="ring", grad="ring"),
    U("layer1_b4", 4, 100, 100, 64, 64, res=True, fwd="ks", grad="ks"),
    U("layer2_b4", 4, 50, 50, 128, 128, fwd="ks", grad="ks"),
    U("layer3_b4_res", 4, 25, 25, 256, 256, res=True, fwd="ks", grad="ks"),
    U("odd_9x7_res_norelu", 1, 9, 7, 64, 64, res=True, relu=False, fwd="tile", grad="tile"),
    U("odd_37x29_weight_only", 1, 37, 29, 64, 64, need=("w",), fwd="tile", grad="tile"),
    U("odd_61x83_x1_only", 1, 61, 83, 64, 128, need=("x1",), fwd="ks", grad="tile"),
    U("up2_skip_30x26_x2_without_x1", 2, 30, 26, 64, 128, C2=64, up=2, need=("x2", "w"), fwd="tile", grad="ks"),
    U("up4_skip_9x7_res", 1, 9, 7, 64, 64, C2=64, up=4, res=True, fwd="tile", grad="tile"),
    U("up2_13x11_norelu", 2, 13, 11, 64, 64, up=2, relu=False, fwd="tile", grad="tile"),
    U("c128_b4_res_without_x1", 4, 100, 100, 128, 64, res=True, need=("res", "w"), fwd="tile", grad="ring"),
    U("ring_ab_200x200", 1, 200, 200, 64, 128, fwd="ring", grad="tile"),
]
RING_AB = "ring_ab_200x200"   # run once more with LSS_CONV_RING=0: tile / tile, same bound

# the unfused nodes: _Conv3x3Fn plain (CONV) and behind the fused upsample + concat (UPCONV) (conv stage only), _BNActFn
# (BatchNorm stage only)
CONV = [
    U("conv_37x29", 1, 37, 29, 64, 64),
    U("conv_9x7_c128", 2, 9, 7, 128, 64),
]
# Cout = 32: the BatchNorm kernels take it, the gradient conv does not (K blocks of 64 channels): the guards send the
# conv to the library (whose weight gradient under bf16 autocast is a bf16 tensor) and the BatchNorm to _BNActFn
COUT32 = U("odd_9x7_cout32_res_norelu", 1, 9, 7, 64, 32, res=True, relu=False)
UPCONV = [
    U("upconv4_skip_9x7", 1, 9, 7, 64, 64, C2=64, up=4),
    U("upconv2_13x11", 2, 13, 11, 64, 64, up=2),
    U("upconv2_skip_30x26", 2, 30, 26, 64, 128, C2=64, up=2),
]
BN = [
    U("bn_c64_res", 3, 17, 23, 0, 64, res=True),
    U("bn_c32", 2, 9, 7, 0, 32),
    U("bn_c256_norelu_res", 1, 25, 25, 0, 256, res=True, relu=False),
]
# shapes both the fused node and conv node + _BNActFn take
FUSED_VS_UNFUSED = [FUSED[8], FUSED[10], FUSED[11], U("plain_37x29_res", 1, 37, 29, 64, 64, res=True)]

DEGENERATE = U("degenerate_channels", 2, 21, 19, 64, 64)
ZERO_GRAD = U("zero_upstream_gradient", 1, 21, 19, 64, 64, res=True)
ONE_ROW = U("one_row", 1, 1, 1, 0, 64, res=True)     # BatchNorm stage alone: M = 1

# _ConvS2Fn: (name, K, B, H, W, C, Cout, weight gradient on the native K9w kernel?)
S2 = [
    ("s2_k3_36x44", 3, 2, 36, 44, 64, 64, True),
    ("s2_k1_36x44", 1, 2, 36, 44, 64, 128, True),
    ("s2_k7_40x56", 7, 1, 40, 56, 64, 64, True),
    ("s2_k3_12x12_gemm_wgrad", 3, 2, 12, 12, 64, 64, False),   # W // 2 = 6 < 8: _s2_wgrad_native_ok is false
    ("s2_k7_12x12_gemm_wgrad", 7, 1, 12, 12, 64, 64, False),
]


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def make_operands(u, seed=None):
    """CPU operands of a unit: activations and the upstream gradient as fp32 tensors holding bf16 values (NCHW), the
    fp32 parameters as the modules hold them.  x1 has a non-zero mean so that channel means are not negligible."""
    g = torch.Generator().manual_seed(sum(ord(c) for c in u.name) if seed is None else seed)
    Hh, Wh = u.H * u.up, u.W * u.up
    op = {"unit": u, "up": u.up, "stride": 1, "pad": 1}
    if u.Cx:
        op["x1"] = bf16_round(torch.randn(u.B, u.Cx, u.H, u.W, generator=g) + 0.25)
        op["x2"] = bf16_round(torch.randn(u.B, u.C2, Hh, Wh, generator=g)) if u.C2 else None
        Ct = u.Cx + u.C2
        op["w"] = torch.randn(u.Cout, Ct, 3, 3, generator=g) / (3 * Ct ** 0.5)
    else:
        op["z"] = bf16_round(torch.randn(u.B, u.Cout, Hh, Wh, generator=g) * 2 + 0.5)
    # gamma in [0.75, 1.5], beta ~ 0.25 + 0.2 randn: with these the ReLU band holds less than 5 % of the elements also
    # for the units without a residual (gamma from 0.5 and beta about 0 put 5.04 % there at up1.conv0's size)
    op["gamma"] = torch.rand(u.Cout, generator=g) * 0.75 + 0.75
    op["beta"] = torch.randn(u.Cout, generator=g) * 0.2 + 0.25
    op["res"] = bf16_round(torch.randn(u.B, u.Cout, Hh, Wh, generator=g)) if u.res else None
    op["gy"] = bf16_round(torch.randn(u.B, u.Cout, Hh, Wh, generator=g))
    op["running_mean"] = torch.randn(u.Cout, generator=g) * 0.1
    op["running_var"] = torch.rand(u.Cout, generator=g) + 0.5
    op["relu"], op["bn"] = u.relu, True
    return op


def make_s2_operands(name, K, B, H, W, C, Co):
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    return {"x1": bf16_round(torch.randn(B, C, H, W, generator=g) + 0.25), "x2": None, "up": 1, "stride": 2, "pad": K // 2,
            "w": torch.randn(Co, C, K, K, generator=g) / (K * C ** 0.5), "res": None, "bn": False, "relu": False,
            "gy": bf16_round(torch.randn(B, Co, H // 2, W // 2, generator=g))}


def _upsample(x, up):
    return F.interpolate(x, scale_factor=up, mode="bilinear", align_corners=True)


def _upsample_adjoint(g, up):
    B, C, Hh, Wh = g.shape
    x = torch.zeros(B, C, Hh // up, Wh // up, dtype=g.dtype, requires_grad=True)
    return torch.autograd.grad(_upsample(x, up), x, g)[0]


def _bn_stats(z, op, dtype):
    C = z.shape[1]
    M = z.numel() // C
    mean = z.mean((0, 2, 3))
    var = z.var((0, 2, 3), unbiased=False)
    # M = 1: torch refuses training-mode statistics of one value; the variance of one value is 0 and there is no
    # unbiased estimate, so the running variance moves towards 0 (what the kernels document)
    unbiased = var * (M / (M - 1.0)) if M > 1 else var
    rm = (1 - MOMENTUM) * op["running_mean"].to(dtype) + MOMENTUM * mean
    rv = (1 - MOMENTUM) * op["running_var"].to(dtype) + MOMENTUM * unbiased
    return M, mean, var, rm, rv


def reference(op, mask=None):
    """fp64 torch + autograd.  mask: None = forward only (or no ReLU); else the 0/1 tensor of the backward's ReLU."""
    dt = torch.float64
    leaf = lambda t: None if t is None else t.detach().to(dt).requires_grad_(True)  # noqa: E731
    out, leaves = {}, {}
    if op.get("w") is not None:
        x1, x2 = leaf(op["x1"]), leaf(op["x2"])
        w = leaf(op["w"].to(torch.bfloat16))
        xu = _upsample(x1, op["up"]) if op["up"] > 1 else x1
        xc = xu if x2 is None else torch.cat([x2, xu], 1)
        z = F.conv2d(xc, w, stride=op["stride"], padding=op["pad"])
        leaves.update(g1=x1, g2=x2, dw=w)
    else:
        z = leaf(op["z"])
    leaves["dz"] = z
    out["z"] = z.detach()
    if op["bn"]:
        gamma, beta, res = leaf(op["gamma"]), leaf(op["beta"]), leaf(op["res"])
        M, mean, var, rm, rv = _bn_stats(z.detach(), op, dt)
        if M > 1:
            rm_t, rv_t = op["running_mean"].to(dt).clone(), op["running_var"].to(dt).clone()
            t = F.batch_norm(z, rm_t, rv_t, gamma, beta, True, MOMENTUM, EPS)
            assert torch.allclose(rm_t, rm, rtol=1e-12, atol=1e-14) and torch.allclose(rv_t, rv, rtol=1e-12, atol=1e-14)
        else:
            t = gamma.view(1, -1, 1, 1) * (z - z.mean((0, 2, 3), keepdim=True)) * (0 * z + EPS).rsqrt() + beta.view(1, -1, 1, 1)
        if res is not None:
            t = t + res
        out.update(mean=mean, invstd=(var + EPS).rsqrt(), running_mean=rm, running_var=rv)
        leaves.update(dgamma=gamma, dbeta=beta, dres=res)
    else:
        t = z
    out["t"] = t.detach()
    out["y"] = torch.relu(t.detach()) if op["relu"] else t.detach()
    if op["relu"] and mask is None:
        return out
    yb = t * mask.to(dt) if op["relu"] else t
    keys = [k for k, v in leaves.items() if v is not None]
    grads = torch.autograd.grad(yb, [leaves[k] for k in keys], op["gy"].to(dt))
    out.update(zip(keys, grads))
    return out


def evaluate(op, mask=None, emulate=True, plant=None, dtype=None, per_sample_bf16_dw=False, bf16_dw=False,
             col2im_bf16=False):
    """The chain by hand (see the module docstring).  Emulated evaluations run the convs in fp32 by default (their
    1e-6 is far below the bf16 roundings they carry); emulate=False defaults to fp64.  per_sample_bf16_dw: the
    im2col + GEMM weight gradient of the stride-2 conv (one bf16 GEMM per sample, summed in fp32); bf16_dw: a weight
    gradient that is stored in bf16 (the library conv under bf16 autocast); col2im_bf16: the GEMM + col2im input
    gradient of the stride-2 conv (the per-tap columns are a bf16 tensor before they are folded).
    plant: "dgamma_without_mean" | "upsample_adjoint_last_row_dropped" | "unflipped_taps"."""
    dt = dtype or (torch.float32 if emulate else torch.float64)
    r = bf16_round if emulate else (lambda t: t)
    out = {}
    conv = op.get("w") is not None
    if conv:
        x1 = op["x1"].to(dt)
        xu = r(_upsample(x1, op["up"])) if op["up"] > 1 else x1
        xc = xu if op["x2"] is None else torch.cat([op["x2"].to(dt), xu], 1)
        wb = op["w"].to(torch.bfloat16).to(dt)
        z = r(F.conv2d(xc, wb, stride=op["stride"], padding=op["pad"]))
    else:
        z = op["z"].to(dt)
    out["z"] = z
    z = z.double()   # everything per element and per channel in fp64: only the storage roundings are emulated
    if op["bn"]:
        c = lambda v: v.double().view(1, -1, 1, 1)  # noqa: E731
        M, mean, var, rm, rv = _bn_stats(z, op, torch.float64)
        invstd = (var + EPS).rsqrt()
        xhat = (z - c(mean)) * c(invstd)
        t = c(op["gamma"]) * xhat + c(op["beta"])
        if op["res"] is not None:
            t = t + op["res"].double()
        out.update(mean=mean, invstd=invstd, running_mean=rm, running_var=rv)
    else:
        t = z
    out["t"] = t
    out["y"] = r(torch.relu(t) if op["relu"] else t)
    if op["relu"] and mask is None:
        return out
    g = op["gy"].double() * (mask.double() if op["relu"] else 1.0)
    if op["bn"]:
        dbeta = g.sum((0, 2, 3))
        dgamma = (g * xhat).sum((0, 2, 3))
        dz = r(c(op["gamma"]) * c(invstd) * (g - c(dbeta) / M - xhat * c(dgamma) / M))
        if plant == "dgamma_without_mean":
            dgamma = (g * z * c(invstd)).sum((0, 2, 3))
        out.update(dbeta=dbeta, dgamma=dgamma, dz=dz)
        if op["res"] is not None:
            out["dres"] = r(g)
    else:
        dz = out["dz"] = g
    if conv:
        dzc = dz.to(dt)
        wd = wb.flip(2, 3) if plant == "unflipped_taps" else wb
        if col2im_bf16:
            Bn, Co, K = dzc.shape[0], wd.shape[0], wd.shape[2]
            cols = r(torch.matmul(wd.reshape(Co, -1).t(), dzc.reshape(Bn, Co, -1)))
            gcat = r(F.fold(cols, xc.shape[2:], K, padding=op["pad"], stride=op["stride"]))
        else:
            gcat = r(torch.nn.grad.conv2d_input(xc.shape, wd, dzc, stride=op["stride"], padding=op["pad"]))
        C2 = 0 if op["x2"] is None else op["x2"].shape[1]
        if C2:
            out["g2"] = gcat[:, :C2]
        gu = gcat[:, C2:]
        if op["up"] > 1:
            if plant == "upsample_adjoint_last_row_dropped":
                gu = gu.clone()
                gu[:, :, -1] = 0
            out["g1"] = r(_upsample_adjoint(gu, op["up"]))
        else:
            out["g1"] = gu
        if per_sample_bf16_dw:
            out["dw"] = sum(bf16_round(torch.nn.grad.conv2d_weight(xc[b:b + 1], wb.shape, dzc[b:b + 1], stride=op["stride"],
                                                                    padding=op["pad"])) for b in range(xc.shape[0]))
        else:
            out["dw"] = torch.nn.grad.conv2d_weight(xc, wb.shape, dzc, stride=op["stride"], padding=op["pad"])
            if bf16_dw:
                out["dw"] = r(out["dw"])
    return out


def errors(a, b):
    """(max |a - b| / max |b|, ||a - b|| / ||b||); a reference that is exactly 0 admits only exactly 0."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    d = a - b
    if not bool(torch.isfinite(d).all()):
        return float("inf"), float("inf")
    dm, bm = float(d.abs().max()) if d.numel() else 0.0, float(b.abs().max()) if b.numel() else 0.0
    if bm == 0.0:
        e = 0.0 if dm == 0.0 else float("inf")
        return e, e
    return dm / bm, float(d.norm() / b.norm())


def minimum(key):
    return MIN_BF16 if key in BF16_OUTPUTS else MIN_F32


def floors(ref, emu, keys=None):
    """{output: (floor_max, floor_l2)} of the outputs both evaluations hold."""
    return {k: errors(emu[k], ref[k]) for k in (keys or ref) if k in emu and k in ref and k != "t"}


def bounds(floor):
    return {k: tuple(max(FACTOR * f, minimum(k)) for f in fl) for k, fl in floor.items()}


def band_fraction(ref):
    band = BAND_SCALE * float(ref["y"].abs().max())
    return float((ref["t"].abs() <= band).double().mean()), band


def mask_check(y_kernel, ref):
    """The ReLU decisions of the node's own output against the fp64 pre-activation: exact outside the band, and the band
    holds at most 5 % of the elements.  Returns (fraction in the band, decisions that differ inside it)."""
    frac, band = band_fraction(ref)
    assert frac <= BAND_MAX_FRACTION, "the band hides %.2f %% of the elements" % (100 * frac)
    mk, mr = y_kernel.detach().cpu() > 0, ref["t"] > 0
    outside = ref["t"].abs() > band
    wrong = int((mk != mr)[outside].sum())
    assert wrong == 0, "%d ReLU decisions outside the band differ from the fp64 reference" % wrong
    return frac, int((mk != mr).sum())


def make_degenerate_operands():
    """Channel 0: all-zero weights -> constant z, variance 0.  Channel 1: beta = -10 -> y <= 0 everywhere, mask all zero.
    Channel 2: gamma = 0 (the zero_init_residual state of every fresh model).  The constant pre-activations of channels
    0 and 2 are kept out of the ReLU band."""
    op = make_operands(DEGENERATE)
    op["w"][0] = 0.0
    op["beta"][0], op["beta"][1], op["beta"][2] = 0.5, -10.0, 0.5
    op["gamma"][2] = 0.0
    return op


def make_zero_grad_operands():
    op = make_operands(ZERO_GRAD)
    op["gy"].zero_()
    return op


# (mean, std) of channels 1 .. 17 of the shared-pivot statistics case; the first LARGE_MEAN_ASSERTED (|mean| / std up to
# 10) must keep invstd within 2e-4, the rest are measured and reported
LARGE_MEAN = [(2.0, 1.0), (-2.0, 1.0), (4.0, 1.0), (-4.0, 1.0), (6.0, 1.0), (-6.0, 1.0), (8.0, 1.0), (-8.0, 1.0),
              (10.0, 1.0), (-10.0, 1.0), (10.0, 10.0), (20.0, 1.0), (-50.0, 1.0), (100.0, 1.0), (300.0, 2.0), (-2000.0, 8.0)]
LARGE_MEAN_ASSERTED = 11
SMALL_GAMMA = U("small_gamma_37x29", 1, 37, 29, 64, 64)


def make_small_gamma_operands():
    """gamma in [0.02, 0.12]: small scales other than the exact 0 of the degenerate case."""
    op = make_operands(SMALL_GAMMA)
    op["gamma"] = (op["gamma"] - 0.75) / 0.75 * 0.1 + 0.02
    return op


SPLIT_BN = [(2, True, True), (3, True, True), (3, False, False)]   # shards, relu, residual


def make_split_bn_operands(shards, C=64, relu=True, res=True, large=False, H=20, W=24):
    """A batch of `shards` x 2 samples whose shards have different statistics.  large: the channels of LARGE_MEAN
    (mean, std) - unit spread with |mean| = 2 .. 10 in both signs, 10 / 10, then ratios of 20, 50 and 100 and the
    300 / 2 and -2000 / 8 channels of the local-pivot cancellation test - in channels 1 .. len(LARGE_MEAN), drawn
    with the same statistics in every shard."""
    u = U("split_bn_%d%s" % (shards, "_large" if large else ""), 2 * shards, H, W, 0, C, res=res, relu=relu)
    op = make_operands(u)
    z = (op["z"] - 0.5) / 2
    base = z.clone()   # mean 0, std 1
    for s in range(shards):
        z[2 * s:2 * s + 2] = z[2 * s:2 * s + 2] * (1.0 + 0.5 * s) + 0.5 * s
    if large:
        for k, (m, s) in enumerate(LARGE_MEAN, 1):
            z[:, k] = m + s * base[:, k]
    op["z"] = bf16_round(z)
    op["running_mean"] = torch.zeros(C)   # a fresh model: the shared pivot of the split form
    op["running_var"] = torch.ones(C)
    return op
