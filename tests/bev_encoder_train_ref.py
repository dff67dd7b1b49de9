"""fp64 references, rounding floors, plants and cases for the native training route of `BEVEncoderTransformer`
(tests/test_bev_encoder_train_gpu.py on the GPU, tests/test_bev_encoder_train_ref_cpu.py for this helper itself).

Three pieces, each restated from its formulas and held against torch's own fp64 autograd by the CPU tests:

  the biased 3x3 unit   conv3x3(bias) -> BatchNorm(train) -> ReLU.  A train-mode BatchNorm removes a per-channel
                        constant: with z' = conv(x) WITHOUT the bias, y, the saved statistics, running_var and every
                        gradient are those of the bias-free unit of tests/train_node_ref.py; running_mean holds
                        m * b more, and the gradient of b is exactly 0.
  the 1x1 unit          the same with a 1x1 conv (pad 0): `compress`.
  the head              logit[p][k] = b[k] + sum_c y[p][c] W[k][c] over bf16 rows y of 64 channels, alone (forward,
                        backward from a given gradient of the logits) and fused with the weighted cross-entropy
                        loss = sum_p w[t_p] (lse_p - logit[p][t_p]) / sum_p w[t_p] over the pixels with t_p in [0, K).

Bounds.  Units: `train_node_ref.FACTOR` x the rounding floor (the distance of the bf16 emulation - operands and z
rounded where the kernels round, fp32 accumulation - from the fp64 reference), with train_node_ref's minimums.  Head:
the bounds of the 128-channel tests (tests/test_modules_gpu.py): logits 1e-5, loss 2e-5, dy one bf16 rounding (2^-8),
dW / db 2e-4, all max |a - b| / max |b|.

Plants (wrong copies the bounds have to reject): running_mean without the m * b term, running_mean with b instead of
m * b, a bias gradient sum(dy) (the formula of a conv that no BatchNorm follows), and a head whose pixel sum takes in the
neighbouring pixel's lanes (the fourth DPP step of the 128-channel kernel applied to 8-lane pixels)."""
import torch
from torch.nn import functional as F

import train_node_ref as R

U = R.U
# `_train_conv_bn_act` with a biased conv.  W = 6 is below the K9w weight-gradient kernel's width: the GEMM form.
BIASED_3X3 = [
    U("biased_64_64", 2, 12, 16, 64, 64),
    U("biased_128_64", 2, 12, 16, 128, 64),
    U("biased_256_128", 2, 12, 16, 256, 128),
    U("biased_64_64_w6_gemm_wgrad", 2, 12, 6, 64, 64),
]
# ring-eligible (384 strips of 20 x 4): compared against LSS_CONV_RING=0, at the bound of the same widths' small case
RING = U("biased_256_128_ring_96x160", 2, 96, 160, 256, 128)
RING_FLOOR_FROM = "biased_256_128"
CONV_1X1 = [
    U("compress_64_256", 2, 10, 10, 64, 256),
    U("compress_128_256", 2, 10, 10, 128, 256),
]
UNIT_OUTPUTS = ("y", "z", "mean", "invstd", "running_mean", "running_var", "g1", "dw", "dgamma", "dbeta")

HEAD_BOUNDS = {"logits": 1e-5, "loss": 2e-5, "dy": 2.0 ** -8, "dw": 2e-4, "db": 2e-4}
# (name, K, (B, H, W), targets outside [0, K) and a zero-weight class?)
HEAD_CASES = [
    ("ragged_2x5x7_k4", 4, (2, 5, 7), False),
    ("ragged_2x5x7_k8", 8, (2, 5, 7), False),
    ("second_trip_1x136x128_k4", 4, (1, 136, 128), False),   # 17 408 pixels > 512 workgroups x 4 waves x 8 = 16 384
    ("second_trip_1x136x128_k8", 8, (1, 136, 128), False),
    ("ignored_targets_zero_weight_k4", 4, (2, 5, 7), True),
]


def make_unit_operands(u, ksize=3):
    """train_node_ref.make_operands plus a conv bias of the order of z's standard deviation (about 1 with these
    weights: |b| in [0.5, 1.5], both signs), so that a running_mean without m * b, or with b, is far outside the bound.
    ksize = 1: a 1x1 weight with the same scaling (z of unit variance), pad 0."""
    op = R.make_operands(u)
    g = torch.Generator().manual_seed(1000 + sum(ord(c) for c in u.name))
    if ksize == 1:
        op["w"] = torch.randn(u.Cout, u.Cx, 1, 1, generator=g) / u.Cx ** 0.5
        op["pad"] = 0
    sign = (torch.rand(u.Cout, generator=g) < 0.5).float() * 2 - 1
    op["bias"] = sign * (torch.rand(u.Cout, generator=g) + 0.5)
    return op


def unit_reference(op, mask=None):
    """fp64 reference of the biased unit: train_node_ref.reference of the bias-free unit (z is conv(x) without the
    bias, what the kernels store), running_mean + m * b, and the exact zero gradient of the bias."""
    out = R.reference(op, mask)
    out["running_mean"] = out["running_mean"] + R.MOMENTUM * op["bias"].double()
    if "dw" in out:
        out["dbias"] = torch.zeros_like(op["bias"], dtype=torch.float64)
    return out


def unit_evaluate(op, mask=None, emulate=True, plant=None):
    """train_node_ref.evaluate of the bias-free unit with the bias rule on top; emulate: running_mean as the kernels
    form it (fp32: the BatchNorm kernel's update, then one fp32 add of m * b).
    plant: "running_mean_without_bias" | "running_mean_full_bias" | "bias_grad_sum_dy"."""
    out = R.evaluate(op, mask, emulate=emulate)
    b = op["bias"].double()
    add = {None: R.MOMENTUM * b, "bias_grad_sum_dy": R.MOMENTUM * b, "running_mean_without_bias": 0 * b,
           "running_mean_full_bias": b}[plant]
    if emulate:
        out["running_mean"] = (out["running_mean"].float() + add.float()).double()
    else:
        out["running_mean"] = out["running_mean"] + add
    if "dw" in out:
        out["dbias"] = torch.zeros_like(b)
        if plant == "bias_grad_sum_dy":
            g = op["gy"].double() * (mask.double() if op["relu"] else 1.0)
            out["dbias"] = g.sum((0, 2, 3))
    return out


def torch_unit(op):
    """The unit as torch composes it, in fp64 with its own autograd: nn.Conv2d(bias=True) -> nn.BatchNorm2d (train) ->
    ReLU from the same operands (weights rounded to bf16 as the kernels pack them).  Returns the outputs under the
    names of `unit_reference` plus the ReLU mask torch used."""
    u = op["unit"]
    k = op["w"].shape[2]
    conv = torch.nn.Conv2d(u.Cx, u.Cout, k, padding=op["pad"], bias=True).double()
    bn = torch.nn.BatchNorm2d(u.Cout, eps=R.EPS, momentum=R.MOMENTUM).double().train()
    with torch.no_grad():
        conv.weight.copy_(op["w"].to(torch.bfloat16).double())
        conv.bias.copy_(op["bias"].double())
        bn.weight.copy_(op["gamma"].double())
        bn.bias.copy_(op["beta"].double())
        bn.running_mean.copy_(op["running_mean"].double())
        bn.running_var.copy_(op["running_var"].double())
    x = op["x1"].double().requires_grad_(True)
    t = bn(conv(x))
    y = torch.relu(t)
    y.backward(op["gy"].double())
    return {"y": y.detach(), "t": t.detach(), "mask": (t.detach() > 0).double(), "g1": x.grad, "dw": conv.weight.grad,
            "dbias": conv.bias.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
            "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(),
            "num_batches_tracked": int(bn.num_batches_tracked)}


# ---------------------------------------------------------------------------------------------------------------------
# the head over 64-channel rows
# ---------------------------------------------------------------------------------------------------------------------
def make_head_operands(name, K, shape, odd_targets, cin=64):
    """y: what a conv + BatchNorm + ReLU unit hands over (non-negative bf16 values); head weights as nn.Conv2d holds
    them (fp32); class weights in [1, 10]; g: a gradient of the logits for the head-alone backward.  odd_targets: some
    targets are -100 and 255 (ignored), and class 1 has weight 0."""
    B, H, W = shape
    g = torch.Generator().manual_seed(sum(ord(c) for c in name))
    op = {"K": K, "shape": shape,
          "y": R.bf16_round(torch.randn(B, H, W, cin, generator=g).relu()),
          "w": torch.randn(K, cin, generator=g) * cin ** -0.5, "b": torch.randn(K, generator=g) * 0.1,
          "t": torch.randint(0, K, (B, H, W), generator=g), "cw": torch.rand(K, generator=g) * 9 + 1,
          "g": torch.randn(B, K, H, W, generator=g), "gl": 1.7}
    if odd_targets:
        op["t"][0, 0, :3] = -100
        op["t"][1, 2, 1:4] = 255
        op["cw"][1] = 0.0
    return op


def head_evaluate(op, dtype=torch.float64, plant=None):
    """All four modes by hand in `dtype` (fp64: the reference; fp32 with dy rounded to bf16: the emulation).
    Returns logits (B, K, H, W), loss, and for both backwards dy (B, H, W, Cin), dw (K, Cin), db (K):
    `ce_*` for the fused head + cross-entropy (upstream gradient op["gl"]), `h_*` for the head alone (op["g"]).
    plant = "neighbour_lanes": every pixel's dot products take in those of pixel p ^ 1 (a missing pixel counts 0)."""
    K = op["K"]
    y = op["y"].to(dtype)
    Cin = y.shape[-1]
    rows = y.reshape(-1, Cin)
    M = rows.shape[0]
    w, b, cw = op["w"].to(dtype), op["b"].to(dtype), op["cw"].to(dtype)
    dots = rows @ w.t()                                   # (M, K)
    if plant == "neighbour_lanes":
        padded = torch.cat([dots, dots.new_zeros(M % 2, K)])
        dots = dots + padded.view(-1, 2, K).flip(1).reshape(-1, K)[:M]
    logit = dots + b
    B, H, W = op["shape"]
    out = {"logits": logit.view(B, H, W, K).permute(0, 3, 1, 2)}
    # fused head + weighted cross-entropy
    t = op["t"].reshape(-1)
    ok = (t >= 0) & (t < K)
    tc = torch.where(ok, t, torch.zeros_like(t))
    wt = torch.where(ok, cw[tc], cw.new_zeros(()))
    mx = logit.max(1, keepdim=True)[0]
    ex = (logit - mx).exp()
    se = ex.sum(1)
    nll = mx[:, 0] + se.log() - logit.gather(1, tc[:, None])[:, 0]
    sw = wt.sum()
    out["loss"] = (wt * nll).sum() / sw
    onehot = F.one_hot(tc, K).to(dtype) * ok[:, None].to(dtype)
    g_ce = (op["gl"] * wt / sw)[:, None] * (ex / se[:, None] - onehot)
    g_h = op["g"].to(dtype).permute(0, 2, 3, 1).reshape(M, K)
    for tag, g in (("ce", g_ce), ("h", g_h)):
        dy = g @ w
        if dtype != torch.float64:
            dy = R.bf16_round(dy)
        out[tag + "_dy"] = dy.view(B, H, W, Cin)
        out[tag + "_dw"] = g.t() @ rows
        out[tag + "_db"] = g.sum(0)
    return out


def torch_head(op):
    """torch's own fp64 autograd of F.conv2d + F.cross_entropy(weight=...) and of F.conv2d alone, under the names of
    `head_evaluate`.  Targets outside [0, K) are handed to torch as its ignore_index (-100): the kernels ignore all of
    them, torch raises for any other value."""
    K = op["K"]
    out = {}
    t = op["t"].clone()
    t[(t < 0) | (t >= K)] = -100
    for tag in ("ce", "h"):
        y = op["y"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        w = op["w"].double().view(K, -1, 1, 1).clone().requires_grad_(True)
        b = op["b"].double().clone().requires_grad_(True)
        logits = F.conv2d(y, w, b)
        if tag == "ce":
            loss = F.cross_entropy(logits, t, weight=op["cw"].double(), ignore_index=-100)
            (loss * op["gl"]).backward()
            out["logits"], out["loss"] = logits.detach(), loss.detach()
        else:
            logits.backward(op["g"].double())
        out[tag + "_dy"] = y.grad.permute(0, 2, 3, 1)
        out[tag + "_dw"] = w.grad.view(K, -1)
        out[tag + "_db"] = b.grad
    return out


def rel_max(a, b):
    """max |a - b| / max |b| (the metric of the 128-channel head tests)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def head_errors(got, ref):
    """{quantity: error} over the keys of `got`, each against the bound HEAD_BOUNDS[key without its mode prefix]."""
    return {k: rel_max(got[k], ref[k]) for k in got}


def head_bound(key):
    return HEAD_BOUNDS[key.split("_")[-1]]


# ---------------------------------------------------------------------------------------------------------------------
# whole-module rule (tests/test_transformer_grad_gpu.py): the native path may be twice as far from the fp32 middle as the
# bf16 composition is, plus 2^-9 of the tensor's largest element
# ---------------------------------------------------------------------------------------------------------------------
def module_distance(a, middle):
    a, middle = a.detach().double().cpu(), middle.detach().double().cpu()
    return float((a - middle).abs().max()), float(middle.abs().max())


def module_within(native, composition, middle):
    """(ok, native distance, composition distance, allowance) under the rule above."""
    dn, scale = module_distance(native, middle)
    dc, _ = module_distance(composition, middle)
    allow = 2.0 * dc + 2.0 ** -9 * scale
    return dn <= allow, dn, dc, allow
