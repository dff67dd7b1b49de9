"""tests/depth_fuse_train_ref.py against torch's own fp64 autograd, and its bounds against its plants (no GPU).

The formulas and torch's fp64 composition differ by fp64 rounding only: 1e-10 of each tensor's largest element is
asked (measured: <= 3e-14)."""
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import depth_fuse_train_ref as T

IDS = [c.name for c in T.CASES]


def torch_tail(op):
    """F.interpolate + cat + nn.Conv2d + nn.BatchNorm2d.train() + ReLU in fp64 with torch's autograd."""
    c = op["case"]
    conv = nn.Conv2d(2 * c.D, c.D, 1).double()
    bn = nn.BatchNorm2d(c.D, eps=T.EPS, momentum=T.MOMENTUM).double().train()
    with torch.no_grad():
        conv.weight.copy_(op["w"].double().view(c.D, 2 * c.D, 1, 1))
        conv.bias.copy_(op["bias"].double())
        bn.weight.copy_(op["gamma"].double())
        bn.bias.copy_(op["beta"].double())
        bn.running_mean.copy_(op["running_mean"].double())
        bn.running_var.copy_(op["running_var"].double())
    d3 = op["d3"].double().requires_grad_(True)
    d4 = op["d4"].double().requires_grad_(True)
    z = conv(torch.cat([d3, F.interpolate(d4, size=(c.H, c.W), mode="bilinear", align_corners=False)], 1))
    t = bn(z)
    u = torch.relu(t)
    u.backward(op["du"].double())
    return {"z": z.detach(), "t": t.detach(), "u": u.detach(), "dd3": d3.grad, "dd4": d4.grad,
            "dw": conv.weight.grad.view(c.D, 2 * c.D), "dbias": conv.bias.grad, "dgamma": bn.weight.grad,
            "dbeta": bn.bias.grad, "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(),
            "num_batches_tracked": int(bn.num_batches_tracked)}


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_formulas_equal_torch_fp64_autograd(case):
    op = T.make_operands(case)
    ref, want = T.reference(op), torch_tail(op)
    assert want["num_batches_tracked"] == 1
    for k in ("z", "t", "u", "dd3", "dd4", "dw", "dgamma", "dbeta", "running_mean", "running_var"):
        err = float((ref[k] - want[k]).abs().max()) / float(want[k].abs().max())
        assert err <= 1e-10, (k, err)
    # torch's bias gradient is the rounding noise of an exact zero; the reference holds the zero
    assert float(want["dbias"].abs().max()) <= 1e-10 * float(want["dw"].abs().max())
    assert int(torch.count_nonzero(ref["dbias"])) == 0
    assert T.accepted(ref, ref)


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_reference_under_a_given_mask(case):
    """With the mask handed in, u and the gradients follow that mask: an all-ones mask gives the tail without ReLU."""
    op = T.make_operands(case)
    ones = torch.ones_like(op["d3"])
    ref = T.reference(op, mask=ones)
    assert torch.equal(ref["u"], ref["t"])
    assert float((ref["dbeta"] - op["du"].double().sum((0, 2, 3))).abs().max()) <= 1e-12 * case.BN * case.H * case.W


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_band_holds_few_elements(case):
    frac, width = T.band(T.reference(T.make_operands(case)))
    print("%s: %.4f %% of the elements within %.3e of the ReLU's edge" % (case.name, 100 * frac, width))
    assert frac <= T.BAND_MAX_FRACTION


@pytest.mark.parametrize("plant", T.PLANTS)
def test_bounds_reject_the_plants(plant):
    """Every plant is rejected on every case, with two exceptions that lie in the plants, not in the bounds: the
    single-pass fp32 variance is wrong only where the mean dwarfs the spread and must be rejected on the "large mean"
    case; the running variance without M / (M - 1) is off by m var / (M - 1), which at the workload maps' M = 528 is
    1.9e-4 of the running variance - below the rule's 2.2e-4 - and must be rejected on the seven cases with M <= 70."""
    missed = []
    for case in T.CASES:
        op = T.make_operands(case)
        ref = T.reference(op)
        bad = T.reference(op, plant=plant)
        d = T.devs(bad, ref)
        worst = max(d, key=d.get)
        print("%-28s %-24s worst %-13s dev %.3g, d(b) non-zeros %d"
              % (plant, case.name, worst, d[worst], int(torch.count_nonzero(bad["dbias"]))))
        excused = ((plant == "single_pass_variance_fp32" and case.name != T.LARGE_MEAN)
                   or (plant == "running_var_biased" and case.name == "workload_maps"))
        if not excused and T.accepted(bad, ref):
            missed.append(case.name)
    assert not missed, (plant, missed)


def test_torch_fp32_composition_sits_well_inside_the_bound():
    """The composition the kernels replace, in fp32 on the CPU, against the fp64 reference under its own mask: the
    rule leaves it a wide margin on the seven cases of unit level (measured: worst dev 0.006 - 0.02), so the rule needs
    no fitting.  On "large mean" with these operands (channel means up to 144 against a spread of 1) the composition's
    statistics hold (running_var 0.008, dgamma 0.18) but its u sits at 0.76 and its dW at 8.6: z is rounded at the
    level of the mean, and dW = sum dz (x) x multiplies the rounding noise of sum dz (exactly 0) by x ~ 100.  That is
    printed, not asserted; the kernels sum W (x - x0) and dz (x) (x - x0) instead and are held to the rule there too."""
    worst = 0.0
    for case in T.CASES:
        op = T.make_operands(case)
        c = case
        conv = nn.Conv2d(2 * c.D, c.D, 1)
        bn = nn.BatchNorm2d(c.D, eps=T.EPS, momentum=T.MOMENTUM).train()
        with torch.no_grad():
            conv.weight.copy_(op["w"].view(c.D, 2 * c.D, 1, 1))
            conv.bias.copy_(op["bias"])
            bn.weight.copy_(op["gamma"])
            bn.bias.copy_(op["beta"])
            bn.running_mean.copy_(op["running_mean"])
            bn.running_var.copy_(op["running_var"])
        d3, d4 = op["d3"].clone().requires_grad_(True), op["d4"].clone().requires_grad_(True)
        u = torch.relu(bn(conv(torch.cat([d3, F.interpolate(d4, size=(c.H, c.W), mode="bilinear",
                                                            align_corners=False)], 1))))
        u.backward(op["du"])
        got = {"u": u.detach(), "dd3": d3.grad, "dd4": d4.grad, "dw": conv.weight.grad.view(c.D, 2 * c.D),
               "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
               "running_var": bn.running_var}
        T.mask_check(got["u"], T.reference(op))
        ref = T.reference(op, mask=(got["u"] > 0))
        d = {k: T.dev(got[k], ref[k]) for k in got}
        print("%-24s fp32 composition: worst dev %.4f" % (case.name, max(d.values())))
        if case.name == T.LARGE_MEAN:
            print("   " + " ".join("%s %.3g" % kv for kv in sorted(d.items())))
            assert d["running_var"] <= 0.2 and d["running_mean"] <= 0.2   # the two-pass variance holds
            continue
        worst = max(worst, max(d.values()))
    assert worst <= 0.2
