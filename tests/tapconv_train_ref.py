"""fp64 reference, rounding floor, cases and planted errors for the tests of the tap-list training unit
(tests/test_tapconv_train_gpu.py on the GPU, tests/test_tapconv_train_ref_cpu.py for this helper itself).  The
conventions - metrics, factor, minima, ReLU band - are those of tests/train_node_ref.py and are taken from there.

One unit is  act(BatchNorm_train(conv(x, w, ksize, dilation) + b + img_bias[img]))  with ksize 1 or 3, stride 1,
padding = dilation (0 for ksize 1); w is rounded to bf16 as the kernels pack it, b is the conv's own bias (the
train-mode BatchNorm removes it from everything but running_mean).

  reference(op, mask)   plain torch in fp64 (F.conv2d with dilation, F.batch_norm, ReLU) on the bf16-rounded operands;
                        gradients by torch.autograd.grad.  The ReLU of the backward is the multiplication by `mask`.
  evaluate(op, mask, emulate=True, plant=None)
                        the same chain by hand over the LIVE taps only, with bf16 rounding at the storage points z, y,
                        dz, dx.  Its distance from `reference` is the rounding floor of the case; with emulate=False it
                        is an independent second derivation; with `plant=` a deliberately wrong copy.
  wgrad_reference(x, dy, ksize, d) / wgrad_by_taps(..., plant)
                        the weight gradient alone (what lss_tapconv_wgrad computes from bf16 x and dy): autograd through
                        F.conv2d in fp64, and the sum over pixels by hand.
"""
import collections

import torch
from torch.nn import functional as F

import train_node_ref as T

EPS, MOMENTUM = T.EPS, T.MOMENTUM
errors, floors, bounds, band_fraction, mask_check, bf16_round = (T.errors, T.floors, T.bounds, T.band_fraction,
                                                                 T.mask_check, T.bf16_round)
PLANTS = ("tap_from_neighbour_image", "row_wrap", "dead_tap_nonzero", "ky_kx_swapped", "dilation_ignored",
          "last_partial_block_dropped", "img_bias_wrong_image", "dgrad_unflipped")
BLOCK = 32   # pixels per MFMA step of tapconv_wgrad_kernel: what a partial block is partial of

# the weight-gradient cases of the kernel tests: (BN, H, W, Cin, Cout, ksize, dilation)
WGRAD_CASES = [
    (2, 5, 9, 64, 64, 3, 1),        # nine live taps, 90 pixels: a partial last block
    (3, 5, 9, 128, 64, 3, 4),       # nine live taps with row-wrap positions
    (2, 5, 9, 64, 128, 3, 6),       # 1 x 3
    (2, 5, 9, 64, 64, 3, 9),        # centre only
    (1, 1, 1, 64, 64, 3, 1),        # a single pixel
    (2, 8, 22, 768, 256, 3, 2),     # production: the dilated pyramid branch
    (2, 8, 22, 256, 256, 3, 12),    # production: the first atrous conv, 1 x 3 at 8 x 22
    (2, 8, 22, 1024, 256, 1, 1),    # production: the projection
]

Unit = collections.namedtuple("Unit", "name BN H W Cin Cout k d relu conv_bias img_bias")

UNITS = [
    Unit("k3_d2", 3, 5, 9, 128, 64, 3, 2, True, False, False),
    Unit("k3_d6", 3, 5, 9, 128, 64, 3, 6, True, False, False),
    Unit("k1_img_bias", 2, 5, 9, 128, 64, 1, 1, True, False, True),
    Unit("k3_d2_conv_bias", 2, 5, 9, 64, 64, 3, 2, True, True, False),
    Unit("k3_d4_norelu", 2, 5, 9, 64, 128, 3, 4, False, False, False),
]


def live_taps(H, W, ksize, dilation):
    """Taps ky * 3 + kx whose shift stays inside an (H, W) map for at least one pixel; the single tap 0 of a 1x1."""
    if ksize == 1:
        return [0]
    return [3 * (ky + 1) + kx + 1 for ky in (-1, 0, 1) for kx in (-1, 0, 1)
            if abs(ky * dilation) < H and abs(kx * dilation) < W]


def tap_offset(tap, ksize, dilation):
    return ((tap // 3 - 1) * dilation, (tap % 3 - 1) * dilation) if ksize == 3 else (0, 0)


def make_operands(u, seed=None):
    g = torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(u.name)) if seed is None else seed)
    op = {"unit": u, "k": u.k, "d": u.d, "relu": u.relu}
    op["x"] = bf16_round(torch.randn(u.BN, u.Cin, u.H, u.W, generator=g) + 0.25)
    op["w"] = torch.randn(u.Cout, u.Cin, u.k, u.k, generator=g) / (u.k * u.Cin ** 0.5)
    op["b"] = torch.randn(u.Cout, generator=g) * 0.5 if u.conv_bias else None
    op["img_bias"] = torch.randn(u.BN, u.Cout, generator=g) * 0.5 if u.img_bias else None
    op["gamma"] = torch.rand(u.Cout, generator=g) * 0.75 + 0.75      # with these the ReLU band stays below 5 %
    op["beta"] = torch.randn(u.Cout, generator=g) * 0.2 + 0.25
    op["gy"] = bf16_round(torch.randn(u.BN, u.Cout, u.H, u.W, generator=g))
    op["running_mean"] = torch.randn(u.Cout, generator=g) * 0.1
    op["running_var"] = torch.rand(u.Cout, generator=g) + 0.5
    return op


def make_wgrad_operands(case):
    BN, H, W, Cin, Cout, k, d = case
    g = torch.Generator().manual_seed(1000 + sum((i + 1) * v for i, v in enumerate(case)))
    return (bf16_round(torch.randn(BN, Cin, H, W, generator=g) + 0.25), bf16_round(torch.randn(BN, Cout, H, W, generator=g)))


def _conv(x, w, k, d):
    return F.conv2d(x, w, padding=d if k == 3 else 0, dilation=d)


def reference(op, mask=None):
    """fp64 torch + autograd.  mask: None = forward only (or no ReLU); else the 0/1 tensor of the backward's ReLU."""
    dt = torch.float64
    leaf = lambda t: None if t is None else t.detach().to(dt).requires_grad_(True)  # noqa: E731
    x, w = leaf(op["x"]), leaf(op["w"].to(torch.bfloat16))
    ib, b, gamma, beta = leaf(op["img_bias"]), leaf(op["b"]), leaf(op["gamma"]), leaf(op["beta"])
    z0 = _conv(x, w, op["k"], op["d"])
    if ib is not None:
        z0 = z0 + ib[:, :, None, None]
    z = z0 if b is None else z0 + b.view(1, -1, 1, 1)
    rm, rv = op["running_mean"].to(dt).clone(), op["running_var"].to(dt).clone()
    t = F.batch_norm(z, rm, rv, gamma, beta, True, MOMENTUM, EPS)
    out = {"z": z0.detach(), "t": t.detach(), "running_mean": rm, "running_var": rv}
    out["y"] = torch.relu(t.detach()) if op["relu"] else t.detach()
    if op["relu"] and mask is None:
        return out
    yb = t * mask.to(dt) if op["relu"] else t
    leaves = {"g1": x, "dw": w, "dbias": ib, "db": b, "dgamma": gamma, "dbeta": beta, "dz": z0}
    keys = [k for k, v in leaves.items() if v is not None]
    out.update(zip(keys, torch.autograd.grad(yb, [leaves[k] for k in keys], op["gy"].to(dt))))
    return out


def _shifted(x, dy, dx, plant=None):
    """x (BN, C, H, W) read at (h + dy, w + dx): zero outside the map (the contract).  The two read plants break it."""
    BN, C, H, W = x.shape
    if plant == "tap_from_neighbour_image":      # rows past the image's edge come from the image above / below
        tall = x.transpose(0, 1).reshape(1, C, BN * H, W)
        return _shifted(tall, dy, dx).reshape(C, BN, H, W).transpose(0, 1)
    if plant == "row_wrap":                      # the source index is formed on the flattened image
        return _shifted(x.reshape(BN, C, 1, H * W), 0, dy * W + dx).reshape(BN, C, H, W)
    out = torch.zeros_like(x)
    h0, h1, w0, w1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if h0 < h1 and w0 < w1:
        out[:, :, h0:h1, w0:w1] = x[:, :, h0 + dy:h1 + dy, w0 + dx:w1 + dx]
    return out


def wgrad_reference(x, dy, k, d):
    """dw (Cout, Cin, k, k) fp64 by autograd through F.conv2d.  x (BN, Cin, H, W), dy (BN, Cout, H, W)."""
    w = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(_conv(x.double(), w, k, d), w, dy.double())[0]


def wgrad_by_taps(x, dy, k, d, plant=None):
    """The same sum written out per live tap; dead taps are exactly 0."""
    x, dy = x.double(), dy.double()
    BN, Cin, H, W = x.shape
    dw = torch.zeros(dy.shape[1], Cin, k, k, dtype=torch.float64)
    de = 1 if plant == "dilation_ignored" else d
    if plant == "last_partial_block_dropped":
        keep = (H * W) // BLOCK * BLOCK
        dy = dy.clone().reshape(BN, -1, H * W)
        dy[:, :, keep:] = 0
        dy = dy.reshape(BN, -1, H, W)
    for tap in live_taps(H, W, k, de):
        oy, ox = tap_offset(tap, k, de)
        xs = _shifted(x, oy, ox, plant if plant in ("tap_from_neighbour_image", "row_wrap") else None)
        dw.view(dw.shape[0], Cin, k * k)[:, :, tap] = torch.einsum("bohw,bchw->oc", dy, xs)
    if plant == "dead_tap_nonzero":
        for tap in set(range(k * k)) - set(live_taps(H, W, k, d)):
            dw.view(dw.shape[0], Cin, k * k)[:, :, tap] = dw.view(dw.shape[0], Cin, k * k)[:, :, (k * k) // 2]
    if plant == "ky_kx_swapped":
        dw = dw.transpose(2, 3).contiguous()
    return dw


def evaluate(op, mask=None, emulate=True, plant=None):
    """The chain by hand in fp64, bf16 rounding at z, y, dz, dx when `emulate`.  plant: one of PLANTS."""
    r = bf16_round if emulate else (lambda t: t)
    k, d = op["k"], op["d"]
    x = op["x"].double()
    wb = op["w"].to(torch.bfloat16).double()
    BN, Cin, H, W = x.shape
    taps = live_taps(H, W, k, d)
    wt = wb.reshape(wb.shape[0], Cin, k * k)
    z = sum(torch.einsum("bchw,oc->bohw", _shifted(x, *tap_offset(t, k, d)), wt[:, :, t]) for t in taps)
    if op["img_bias"] is not None:
        z = z + op["img_bias"].double()[:, :, None, None]
    z = r(z)
    out = {"z": z}
    c = lambda v: v.double().view(1, -1, 1, 1)  # noqa: E731
    M = z.numel() // z.shape[1]
    mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    invstd = (var + EPS).rsqrt()
    xhat = (z - c(mean)) * c(invstd)
    t = c(op["gamma"]) * xhat + c(op["beta"])
    b = 0.0 if op["b"] is None else op["b"].double()
    out["running_mean"] = (1 - MOMENTUM) * op["running_mean"].double() + MOMENTUM * (mean + b)
    out["running_var"] = (1 - MOMENTUM) * op["running_var"].double() + MOMENTUM * var * (M / (M - 1.0))
    out["t"] = t
    out["y"] = r(torch.relu(t) if op["relu"] else t)
    if op["relu"] and mask is None:
        return out
    g = op["gy"].double() * (mask.double() if op["relu"] else 1.0)
    dbeta = g.sum((0, 2, 3))
    dgamma = (g * xhat).sum((0, 2, 3))
    dz = r(c(op["gamma"]) * c(invstd) * (g - c(dbeta) / M - xhat * c(dgamma) / M))
    out.update(dbeta=dbeta, dgamma=dgamma, dz=dz)
    sign = 1 if plant == "dgrad_unflipped" else -1
    dx = torch.zeros_like(x)
    for tp in taps:
        oy, ox = tap_offset(tp, k, d)
        dx = dx + _shifted(torch.einsum("bohw,oc->bchw", dz, wt[:, :, tp]), sign * oy, sign * ox)
    out["g1"] = r(dx)
    out["dw"] = wgrad_by_taps(x, dz, k, d, plant)
    if op["img_bias"] is not None:
        out["dbias"] = dz.sum((2, 3))
        if plant == "img_bias_wrong_image":
            out["dbias"] = out["dbias"].roll(1, 0)
    return out
