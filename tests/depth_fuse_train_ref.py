"""fp64 formulas, cases, bounds and plants for the training-mode fusion tail of `MultiScaleDepthNet`
(csrc/depth_fuse_train.hip, `ops.depth_fuse_train_fwd` / `_bwd`, `_DepthFuseFn`): tests/test_depth_heads_train_gpu.py
on the GPU, tests/test_depth_fuse_train_ref_cpu.py for this helper itself.  No torch autograd in here.

For d3 (BN,D,H,W), d4 (BN,D,H4,W4), M = BN H W:
    x[p] = [d3[p], up(d4)[p]]             up = ATen's bilinear, align_corners=False: separable, rows Uh (H x H4), Uw (W x W4)
    z = W x + b                            the conv bias stays in z
    mean, var (biased) over M;  invstd = 1 / sqrt(var + eps);  t = gamma (z - mean) invstd + beta;  u = relu(t)
    running_mean = (1 - m) rm + m mean;  running_var = (1 - m) rv + m var M / (M - 1)
    g = du [mask];  zh = (z - mean) invstd;  dbeta = sum g;  dgamma = sum g zh
    dz = gamma invstd (g - dbeta / M - zh dgamma / M)
    dW = sum_p dz (x) x;  d(d3) = (W^T dz)[:D];  d(d4) = Uh^T (W^T dz)[D:] Uw;  d(b) = 0 exactly
`mask` is the ReLU decision: the reference's own (t > 0) or one handed in (the kernel's), so that gradients are compared
under the same decisions.

Bound: the project's rule for fp32-accumulated kernels against fp64, dev(a) = max |a - ref| / (2e-5 max|ref| + 2e-4 |ref|)
<= 1 (tests/test_vovnet_lift_grad_gpu.py), for every output of CHECKED; d(b) must be a tensor of exact zeros.  ReLU
decisions must equal the reference's outside the band |t_ref| <= 2^-18 max|u_ref|, which may hold at most 1 % of the
elements.

Plants (wrong copies the bounds have to reject, `reference(op, plant=...)`):
    single_pass_variance_fp32   var = E[z^2] - E[z]^2 accumulated in fp32 (rejected on the "large mean" case)
    running_var_biased          running variance without M / (M - 1)
    dz_without_dgamma_term      dz = gamma invstd (g - dbeta / M)
    upT_drops_clamped_tap       the adjoint of the upsample forgets the upper tap where it is clamped onto the lower one
    bias_grad_sum_dz            d(b) = sum dz (rounding noise instead of zeros)
"""
import collections

import torch

EPS, MOMENTUM = 1e-5, 0.1
BAND_SCALE = 2.0 ** -18
BAND_MAX_FRACTION = 0.01
CHECKED = ("u", "mean", "invstd", "running_mean", "running_var", "dd3", "dd4", "dw", "dgamma", "dbeta")
PLANTS = ("single_pass_variance_fp32", "running_var_biased", "dz_without_dgamma_term", "upT_drops_clamped_tap",
          "bias_grad_sum_dz")

Case = collections.namedtuple("Case", "name BN D H W H4 W4 shift")
CASES = [
    Case("small_model_maps", 2, 41, 4, 6, 2, 3, 0.0),
    Case("odd_sizes_ratio_not_2", 2, 41, 5, 7, 3, 4, 0.0),
    Case("workload_maps", 3, 41, 8, 22, 4, 11, 0.0),
    Case("every_lane_live", 2, 64, 3, 5, 2, 2, 0.0),
    Case("d_8", 2, 8, 4, 6, 2, 3, 0.0),
    Case("both_taps_clamped", 2, 41, 4, 6, 1, 1, 0.0),
    Case("m_9", 1, 41, 3, 3, 2, 2, 0.0),
    Case("large_mean", 2, 41, 4, 6, 2, 3, 100.0),      # d3 + 100: the channel means dwarf the spread
]
LARGE_MEAN = "large_mean"


def make_operands(c):
    """fp32 CPU operands: logits of unit scale (d3 shifted by c.shift), a fusion weight that keeps z at unit scale, a
    bias of the order of z's spread, gamma in [0.5, 1.5], beta of both signs (so the ReLU cuts near the middle),
    non-trivial running statistics and an upstream gradient."""
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c.name))
    D = c.D
    return {
        "case": c,
        "d3": torch.randn(c.BN, D, c.H, c.W, generator=g) + c.shift,
        "d4": torch.randn(c.BN, D, c.H4, c.W4, generator=g),
        "w": torch.randn(D, 2 * D, generator=g) / (2 * D) ** 0.5,
        "bias": torch.randn(D, generator=g),
        "gamma": torch.rand(D, generator=g) + 0.5,
        "beta": torch.randn(D, generator=g) * 0.5,
        "running_mean": torch.randn(D, generator=g) * 0.1,
        "running_var": torch.rand(D, generator=g) + 0.5,
        "du": torch.randn(c.BN, D, c.H, c.W, generator=g),
    }


def resize_matrix(n_out, n_in, drop_clamped_tap=False):
    """(n_out, n_in) fp64 matrix of the 1-D bilinear resize, ATen's area_pixel_compute_source_index with
    align_corners=False: s = max(0, (n_in / n_out) (o + 0.5) - 0.5), taps i0 = floor(s), i1 = min(i0 + 1, n_in - 1)."""
    U = torch.zeros(n_out, n_in, dtype=torch.float64)
    r = n_in / n_out
    for o in range(n_out):
        s = max(0.0, r * (o + 0.5) - 0.5)
        i0 = int(s)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = s - i0
        U[o, i0] += 1.0 - l1
        if not (drop_clamped_tap and i1 == i0):
            U[o, i1] += l1
    return U


def reference(op, mask=None, plant=None):
    """Every quantity of the module docstring in fp64; `t` is the pre-activation the mask is taken from."""
    assert plant is None or plant in PLANTS, plant
    c = op["case"]
    D, M = c.D, c.BN * c.H * c.W
    d3, d4, w = op["d3"].double(), op["d4"].double(), op["w"].double()
    gamma, beta = op["gamma"].double(), op["beta"].double()
    Uh, Uw = resize_matrix(c.H, c.H4), resize_matrix(c.W, c.W4)
    up = torch.einsum("hi,bdij,wj->bdhw", Uh, d4, Uw)
    x = torch.cat([d3, up], 1).permute(0, 2, 3, 1).reshape(M, 2 * D)
    z = x @ w.t() + op["bias"].double()
    mean = z.mean(0)
    if plant == "single_pass_variance_fp32":
        z32 = z.float()
        m1 = z32.sum(0) / M
        var = ((z32 * z32).sum(0) / M - m1 * m1).clamp_min(0).double()
    else:
        var = ((z - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    zh = (z - mean) * invstd
    t = gamma * zh + beta
    unb = var if plant == "running_var_biased" else var * M / (M - 1)

    def nchw(rows, ch):
        return rows.reshape(c.BN, c.H, c.W, ch).permute(0, 3, 1, 2)

    out = {"z": nchw(z, D), "t": nchw(t, D), "mean": mean, "invstd": invstd,
           "running_mean": (1 - MOMENTUM) * op["running_mean"].double() + MOMENTUM * mean,
           "running_var": (1 - MOMENTUM) * op["running_var"].double() + MOMENTUM * unb}
    m = (out["t"] > 0) if mask is None else mask.bool()
    out["u"] = out["t"] * m
    g = (op["du"].double() * m).permute(0, 2, 3, 1).reshape(M, D)
    dbeta = g.sum(0)
    dgamma = (g * zh).sum(0)
    dz = gamma * invstd * (g - dbeta / M - (0 if plant == "dz_without_dgamma_term" else zh * dgamma / M))
    dx = nchw(dz @ w, 2 * D)
    UhT = resize_matrix(c.H, c.H4, plant == "upT_drops_clamped_tap")
    UwT = resize_matrix(c.W, c.W4, plant == "upT_drops_clamped_tap")
    out.update(dbeta=dbeta, dgamma=dgamma, dw=dz.t() @ x, dd3=dx[:, :D],
               dd4=torch.einsum("hi,bdhw,wj->bdij", UhT, dx[:, D:], UwT),
               dbias=dz.sum(0) if plant == "bias_grad_sum_dz" else torch.zeros(D, dtype=torch.float64))
    return out


def dev(a, ref):
    """max |a - ref| / (2e-5 max|ref| + 2e-4 |ref|): the rule holds iff dev <= 1."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    scale = 2e-5 * ref.abs().max() + 2e-4 * ref.abs()
    if not float(scale.max()) > 0:
        return 0.0 if not float(a.abs().max()) > 0 else float("inf")
    return float(((a - ref).abs() / scale.clamp_min(1e-300)).max())


def devs(got, ref):
    return {k: dev(got[k], ref[k]) for k in CHECKED}


def accepted(got, ref):
    """The GPU test's verdict on a set of outputs: every CHECKED output within dev <= 1 and d(b) exact zeros."""
    return all(v <= 1.0 for v in devs(got, ref).values()) and int(torch.count_nonzero(got["dbias"])) == 0


def band(ref):
    """(fraction of the elements inside the undecided band, the band's half width)."""
    width = BAND_SCALE * float(ref["u"].abs().max())
    return float((ref["t"].abs() <= width).double().mean()), width


def mask_check(u_kernel, ref):
    """ReLU decisions of the kernel's own output against the fp64 pre-activation: equal outside the band, and the band
    holds at most 1 % of the elements.  Returns (fraction in the band, decisions that differ inside it)."""
    frac, width = band(ref)
    assert frac <= BAND_MAX_FRACTION, "the band hides %.3f %% of the elements" % (100 * frac)
    mk, mr = u_kernel.detach().cpu() > 0, ref["t"] > 0
    outside = ref["t"].abs() > width
    wrong = int(((mk != mr) & outside).sum())
    assert wrong == 0, "%d ReLU decisions differ outside the band" % wrong
    return frac, int((mk != mr).sum())
