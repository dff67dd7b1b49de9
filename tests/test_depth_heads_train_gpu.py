"""Native training of the vovnet depth heads: v2's fusion tail as one node on the kernels of csrc/depth_fuse_train.hip
(`ops.depth_fuse_train_fwd` / `_bwd`, `_DepthFuseFn`), the 3x3 conv-BN-ReLU units of the heads on
`modules._train_conv_bn_act` with the bias absorbed, `_HeadProjFn` on the units' bf16 NHWC output, and the level with
both: route counters, fallbacks, graph capture.

(a) tail kernels against the fp64 formulas of tests/depth_fuse_train_ref.py (held against torch's fp64 autograd, and
    its bounds against its plants, by tests/test_depth_fuse_train_ref_cpu.py): dev <= 1 under the project's rule for
    fp32-accumulated kernels, ReLU decisions exact outside a band of 2^-18 max|u|, d(bias) exact zeros, bit-equal
    repeats, refusals.
(b) head units at the heads' shapes, with the references, floors and bounds of test_biased_3x3_unit_vs_fp64.
(c) `_HeadProjFn` on a bf16 NHWC hidden map against the same node on the fp32 NCHW copy of the same values.
(d) the level under bf16 autocast: native (library conv / interpolate / batch_norm patched to raise) against the bf16
    composition through the fp32 run, `bev_encoder_train_ref.module_within`.
(e) the level in fp32, v2: the tail native, against the fp64 yardstick of test_vovnet_lift_grad_gpu.py.
(f) fallbacks.  (g) capture and replay.
Every measured error is printed and `report`ed before it is asserted.

Measured (MI355X).  Tail kernels, largest dev over the checked outputs: 0.01 (dW) at the workload's maps, 0.19 (dW)
on "large mean" (u 0.12); no ReLU decision differed from the reference's on any case.  `_HeadProjFn` d(hidden) on
bf16 NHWC: 2.2e-3 of its maximum (one bf16 rounding: 3.9e-3), the fp32 gradients bit-equal.  Level, largest native
distance / allowance: v1 0.94, v2 0.50.  Full-width v2 level forward + backward under bf16 autocast at batch 8
(tools/bench_vovnet_lift.py --heads, profiles/r17_depth_heads_train_bench.json), median: both routes native 2.28 ms,
LSS_DEPTH_HEADS_NATIVE=0 alone 2.45 ms (minimum 2.40), LSS_DEPTH_TAIL_NATIVE=0 alone 2.68 ms (minimum 2.62), both off
2.77 ms; peak 359 / 378 / 358 / 377 MiB; the tail alone 9 kernel launches against 32.  The native median lies below
both single-switch minima, so both switches default to on; the tests below select each route
explicitly whatever the defaults.
"""
import copy

import pytest
import torch
from torch import nn

import bev_encoder_train_ref as E
import depth_fuse_train_ref as T
import train_node_ref as R

pytestmark = pytest.mark.gpu

import test_bev_encoder_train_gpu as TB  # noqa: E402  (its unit runner and assertions, used exactly as it uses them)
import test_vovnet_lift_grad_gpu as TL  # noqa: E402  (its models, level runner, yardstick and capture helper)
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# (a) the tail kernels
# ---------------------------------------------------------------------------------------------------------------------
def _tail_gpu(op):
    """Both directions through `ops`; outputs under the reference's names, as the kernels wrote them."""
    dev = {k: op[k].cuda() for k in ("d3", "d4", "w", "bias", "gamma", "beta", "du")}
    rm, rv = op["running_mean"].clone().cuda(), op["running_var"].clone().cuda()
    z, u, mean, invstd = ops.depth_fuse_train_fwd(dev["d3"], dev["d4"], dev["w"], dev["bias"], dev["gamma"],
                                                  dev["beta"], rm, rv, T.MOMENTUM, T.EPS)
    dd3, dd4, dw, dgamma, dbeta = ops.depth_fuse_train_bwd(dev["du"], u, z, dev["d3"], dev["d4"], dev["w"],
                                                           dev["gamma"], mean, invstd)
    torch.cuda.synchronize()
    return {"z": z, "u": u, "mean": mean, "invstd": invstd, "running_mean": rm, "running_var": rv, "dd3": dd3,
            "dd4": dd4, "dw": dw, "dgamma": dgamma, "dbeta": dbeta}


@pytest.mark.parametrize("case", T.CASES, ids=[c.name for c in T.CASES])
def test_tail_kernels_vs_fp64(case, report):
    """u, the saved and the running statistics, d(d3), d(d4), dW, dgamma, dbeta within dev <= 1 of the fp64 formulas
    evaluated under the kernel's own ReLU mask; the mask equals the reference's outside the band; a second call on the
    same inputs is bit-equal."""
    op = T.make_operands(case)
    got = _tail_gpu(op)
    frac, flipped = T.mask_check(got["u"], T.reference(op))
    ref = T.reference(op, mask=(got["u"].cpu() > 0))
    d = T.devs(got, ref)
    for k in T.CHECKED:
        print("tail %-24s %-13s dev %.4f" % (case.name, k, d[k]))
        report("depth_fuse_train.%s.%s" % (case.name, k), d[k])
    print("tail %-24s band holds %.4f %% of the elements, %d decisions differ inside it" % (case.name, 100 * frac, flipped))
    assert all(v <= 1.0 for v in d.values()), {k: v for k, v in d.items() if not v <= 1.0}
    again = _tail_gpu(op)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def _fusion(op):
    c = op["case"]
    f = nn.Sequential(nn.Conv2d(2 * c.D, c.D, 1), nn.BatchNorm2d(c.D, eps=T.EPS, momentum=T.MOMENTUM),
                      nn.ReLU(inplace=True)).cuda().train()
    with torch.no_grad():
        f[0].weight.copy_(op["w"].view(c.D, 2 * c.D, 1, 1))
        f[0].bias.copy_(op["bias"])
        f[1].weight.copy_(op["gamma"])
        f[1].bias.copy_(op["beta"])
        f[1].running_mean.copy_(op["running_mean"])
        f[1].running_var.copy_(op["running_var"])
    return f


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16_autocast"])
def test_tail_node_bias_gradient_counter_and_autocast(monkeypatch, autocast):
    """`_fuse_tail` takes `_DepthFuseFn` with and without autocast (fp32 math either way: the same bits), hands back
    fp32, a bias gradient of exact zeros, the kernels' gradients for every other leaf, and advances
    num_batches_tracked by one."""
    monkeypatch.setenv("LSS_DEPTH_TAIL_NATIVE", "1")
    op = T.make_operands(T.CASES[1])
    f = _fusion(op)
    d3, d4 = op["d3"].cuda().requires_grad_(True), op["d4"].cuda().requires_grad_(True)
    before = dict(mv.FUSE_TAIL_CALLS)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        u = mv._fuse_tail(f, d3, d4)
    assert type(u.grad_fn).__name__ == "_DepthFuseFnBackward" and u.dtype == torch.float32
    assert mv.FUSE_TAIL_CALLS["native"] == before["native"] + 1
    assert mv.FUSE_TAIL_CALLS["composition"] == before["composition"]
    assert int(f[1].num_batches_tracked) == 1
    leaves = [d3, d4, f[0].weight, f[0].bias, f[1].weight, f[1].bias]
    grads = torch.autograd.grad(u, leaves, op["du"].cuda())
    want = _tail_gpu(op)
    assert torch.equal(u.detach(), want["u"])
    for g, k in zip(grads, ("dd3", "dd4", "dw", None, "dgamma", "dbeta")):
        if k is not None:
            assert torch.equal(g.reshape(want[k].shape), want[k]), k
    assert grads[3].dtype == torch.float32 and tuple(grads[3].shape) == (op["case"].D,)
    assert int(torch.count_nonzero(grads[3])) == 0, "fusion.0.bias.grad must be a tensor of exact zeros"
    assert torch.equal(f[1].running_mean, want["running_mean"]) and torch.equal(f[1].running_var, want["running_var"])


def test_tail_refusals_raise_before_any_launch():
    """D = 65, one pixel (nn.BatchNorm2d's own ValueError) and a d4 of another batch size raise ValueError; the
    running statistics - written by the second launch of a forward that started - keep their bits."""
    def call(BN, D, H, W, BN4=None):
        g = torch.Generator().manual_seed(0)
        rm, rv = torch.randn(D, generator=g).cuda(), (torch.rand(D, generator=g) + 0.5).cuda()
        keep = (rm.clone(), rv.clone())
        args = (torch.randn(BN, D, H, W, generator=g).cuda(), torch.randn(BN4 or BN, D, 1, 1, generator=g).cuda(),
                torch.randn(D, 2 * D, generator=g).cuda(), torch.zeros(D).cuda(), torch.ones(D).cuda(),
                torch.zeros(D).cuda(), rm, rv, 0.1, 1e-5)
        with pytest.raises(ValueError) as e:
            ops.depth_fuse_train_fwd(*args)
        torch.cuda.synchronize()
        assert torch.equal(rm, keep[0]) and torch.equal(rv, keep[1])
        return str(e.value)

    call(2, 65, 2, 2)
    assert "Expected more than 1 value per channel when training" in call(1, 8, 1, 1)
    call(2, 8, 2, 2, BN4=3)
    one = torch.ones(1, 8, 1, 1).cuda()
    bn = nn.BatchNorm2d(8).cuda().train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        bn(one)   # the library's words for the same refusal
    L = ops.N.lib()
    p = ops.N.ptr(one)
    assert L.lss_depth_fuse_train_fwd(p, p, p, p, p, p, p, p, 0.1, 1e-5, 1, 8, 1, 1, 1, 1, p, 1 << 20, p, p, p, p,
                                      None) == -2
    assert L.lss_depth_fuse_train_fwd(p, None, p, p, p, p, p, p, 0.1, 1e-5, 2, 8, 1, 1, 1, 1, p, 1 << 20, p, p, p, p,
                                      None) == -1
    assert L.lss_depth_fuse_train_bwd(p, p, p, p, p, p, p, p, p, 2, 65, 1, 1, 1, 1, p, 1 << 20, p, p, p, p, p,
                                      None) == -2
    assert L.lss_depth_fuse_train_workspace_bytes(1 << 16, 8, 1 << 8, 1 << 7) == 0   # BN H W = 2^31


# ---------------------------------------------------------------------------------------------------------------------
# (b) the head units
# ---------------------------------------------------------------------------------------------------------------------
HEAD_UNITS = [
    R.U("head_small_c3_4x6", 2, 4, 6, 128, 256),
    R.U("head_small_c4_2x3_below_the_window", 2, 2, 3, 128, 256),
    R.U("head_c3_8x22_768", 2, 8, 22, 768, 256),
    R.U("head_c4_4x11_1024", 2, 4, 11, 1024, 256),
]


@pytest.mark.parametrize("u", HEAD_UNITS, ids=lambda u: u.name)
def test_head_unit_vs_fp64(u, report):
    """`_train_conv_bn_act` at the depth heads' shapes - 768 -> 256 on 8 x 22, 1024 -> 256 on 4 x 11, the small
    model's 4 x 6 and a 2 x 3 map smaller than the window's reach - exactly as test_biased_3x3_unit_vs_fp64: the fused
    spans, every output within FACTOR x the rounding floor of the fp64 reference of the biased unit, conv.bias.grad
    exact zeros, no flag-wait timeouts."""
    op = E.make_unit_operands(u)
    ops.prepack.clear()
    got, tags, bias_grad, batches = TB._run_unit(op)
    assert TB.FUSED_TAGS <= tags, tags
    TB._assert_bias_rule(bias_grad, op, batches)
    TB._assert_unit(report, u.name, got, op)
    ops.assert_no_timeouts(u.name)


# ---------------------------------------------------------------------------------------------------------------------
# (c) _HeadProjFn on the units' bf16 NHWC output
# ---------------------------------------------------------------------------------------------------------------------
def test_head_proj_on_bf16_nhwc_hidden_map(report):
    """The node fed a bf16 NCHW view over NHWC memory against the same node fed the fp32 NCHW copy of the same values:
    logits and context rows bit-equal (fp32 math on identical operands), the five fp32 gradients within dev <= 1 of
    each other, d(hidden) (bf16, an NCHW view over NHWC memory again) within one bf16 rounding of the fp32 one."""
    g = torch.Generator().manual_seed(31)
    BN, Cd, Cf, D, C, H, W = 2, 256, 64, 41, 128, 4, 6
    base = torch.randn(BN, H, W, Cd, generator=g).relu().to(torch.bfloat16).cuda()
    c3v = torch.randn(BN, Cf, H, W, generator=g).cuda()
    wd, bd = (torch.randn(D, Cd, 1, 1, generator=g) / 16).cuda(), (torch.randn(D, generator=g) * 0.1).cuda()
    wf, bf = (torch.randn(C, Cf, 1, 1, generator=g) / 8).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()
    G1, G2 = torch.randn(BN, D, H, W, generator=g).cuda(), torch.randn(BN, H, W, C, generator=g).cuda()

    def run(hidden_leaf, view):
        leaves = [hidden_leaf] + [t_.clone().requires_grad_(True) for t_ in (wd, bd, c3v, wf, bf)]
        logits, feat = mv._HeadProjFn.apply(view(leaves[0]), *leaves[1:])
        grads = torch.autograd.grad((logits * G1).sum() + (feat * G2).sum(), leaves)
        torch.cuda.synchronize()
        return logits.detach(), feat.detach(), grads

    l16, f16, g16 = run(base.clone().requires_grad_(True), lambda b: b.permute(0, 3, 1, 2))
    l32, f32, g32 = run(base.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True), lambda h: h)
    assert torch.equal(l16, l32) and torch.equal(f16, f32)
    assert g16[0].dtype == torch.bfloat16 and tuple(g16[0].shape) == (BN, H, W, Cd)   # the leaf is the NHWC memory
    dh16, dh32 = g16[0].permute(0, 3, 1, 2).float(), g32[0]
    err = float((dh16 - dh32).abs().max() / dh32.abs().max())
    print("head proj d(hidden): bf16 NHWC vs fp32 NCHW %.3e (one bf16 rounding: %.3e)" % (err, 2.0 ** -8))
    report("head_proj_nhwc.dhidden", err)
    assert err <= 2.0 ** -8
    for name, a, b in zip(("dw_depth", "db_depth", "dc3", "dw_feat", "db_feat"), g16[1:], g32[1:]):
        d = TL.dev(a.cpu(), b.cpu())
        print("head proj %-9s dev %.4f" % (name, d))
        report("head_proj_nhwc." + name, d)
        assert d <= 1.0, (name, d)


# ---------------------------------------------------------------------------------------------------------------------
# (d) - (g) the level
# ---------------------------------------------------------------------------------------------------------------------
def _raiser(name):
    def f(*a, **k):
        raise AssertionError("torch.nn.functional.%s called on the native route" % name)
    return f


def _small(golden, ver):
    g = golden("g10_vovnet_liftsplat_" + ver)
    m = TL.small_model(ver, int(g["seed"])).train()
    calib = [TL.t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    G = torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(3)).cuda()
    return m, TL.t(g["c3"]), TL.t(g["c4"]), calib, G


def _calls():
    return {"heads": dict(mv.HEAD_UNIT_CALLS), "tail": dict(mv.FUSE_TAIL_CALLS), "lift": dict(mv.LIFT_CALLS)}


def _moved(before):
    now = _calls()
    return {k: (now[k]["native"] - before[k]["native"], now[k]["composition"] - before[k]["composition"])
            for k in before}


def _level_step(m, c3, c4, calib, G, autocast):
    """bev, c3.grad, c4.grad and every parameter gradient of the level for loss = sum(bev G); autocast: None (fp32)
    or a dtype."""
    for _, p in TL.level_params(m):
        p.grad = None
    a, b = c3.cuda().requires_grad_(True), c4.cuda().requires_grad_(True)
    with torch.autocast("cuda", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        bev = m.get_voxels(a, b, *calib)
    (bev.float() * G).sum().backward()
    torch.cuda.synchronize()
    out = {"bev": bev.detach().float(), "c3.grad": a.grad}
    if b.grad is not None:
        out["c4.grad"] = b.grad
    out.update({k: p.grad.detach().clone() for k, p in TL.level_params(m)})
    return out


def _pre_bn_biases(ver):
    if ver == "v1":
        return ("depth_net.depth_head.0.bias",)
    return ("depth_net.depth_c3.0.bias", "depth_net.depth_c4.0.bias", "depth_net.fusion.0.bias")


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_level_native_against_composition_through_fp32(golden, monkeypatch, report, ver):
    """Three runs of the small model's train-mode level from one state: fp32 without autocast (the middle), bf16
    autocast with both new switches off, bf16 autocast native with torch.nn.functional.conv2d / interpolate /
    batch_norm patched to raise.  For bev, c3.grad, c4.grad and every parameter gradient:
    max |native - middle| <= 2 max |composition - middle| + 2^-9 max |middle|.  The biases in front of a BatchNorm are
    exact zeros on the native route; v2's depth_c3.3.bias / depth_c4.3.bias (zero by mathematics - the fusion
    BatchNorm removes them -, K10's cancellation noise in practice) are held to 2e-5 max|dW of the same conv|.  The
    counters move by one per unit and tail; the running statistics of every BatchNorm follow the composition's by the
    rule of test_module_running_mean_carries_the_bias."""
    m0, c3, c4, calib, G = _small(golden, ver)
    units = 1 if ver == "v1" else 2
    tails = 0 if ver == "v1" else 1
    monkeypatch.setenv("LSS_DEPTH_HEADS_NATIVE", "1")
    monkeypatch.setenv("LSS_DEPTH_TAIL_NATIVE", "1")
    mid = _level_step(copy.deepcopy(m0), c3, c4, calib, G, None)
    monkeypatch.setenv("LSS_DEPTH_HEADS_NATIVE", "0")
    monkeypatch.setenv("LSS_DEPTH_TAIL_NATIVE", "0")
    mc = copy.deepcopy(m0)
    before = _calls()
    comp = _level_step(mc, c3, c4, calib, G, torch.bfloat16)
    assert _moved(before) == {"heads": (0, units), "tail": (0, tails), "lift": (1, 0)}
    monkeypatch.setenv("LSS_DEPTH_HEADS_NATIVE", "1")
    monkeypatch.setenv("LSS_DEPTH_TAIL_NATIVE", "1")
    for name in ("conv2d", "interpolate", "batch_norm"):
        monkeypatch.setattr(torch.nn.functional, name, _raiser(name))
    mn = copy.deepcopy(m0)
    before = _calls()
    nat = _level_step(mn, c3, c4, calib, G, torch.bfloat16)
    assert _moved(before) == {"heads": (units, 0), "tail": (tails, 0), "lift": (1, 0)}
    zero_by_math = {} if ver == "v1" else {"depth_net.depth_c3.3.bias": "depth_net.depth_c3.3.weight",
                                           "depth_net.depth_c4.3.bias": "depth_net.depth_c4.3.weight"}
    bad, worst = [], 0.0
    for name in sorted(mid):
        if name in _pre_bn_biases(ver):
            assert int(torch.count_nonzero(nat[name])) == 0, name
            continue
        if name in zero_by_math:
            lim = 2e-5 * float(mid[zero_by_math[name]].abs().max())
            ratio = float(nat[name].abs().max()) / lim
            print("level %s %-40s zero by mathematics: |g| / bound %.4f" % (ver, name, ratio))
            if not ratio <= 1.0:
                bad.append((name, ratio, 1.0))
            continue
        ok, dn, dc, allow = E.module_within(nat[name], comp[name], mid[name])
        scale = float(mid[name].abs().max())
        print("level %s %-40s composition %.3e native %.3e" % (ver, name, dc / scale, dn / scale))
        report("depth_heads.level.%s.%s.native" % (ver, name), dn / scale)
        report("depth_heads.level.%s.%s.composition" % (ver, name), dc / scale)
        worst = max(worst, dn / allow)
        if not ok:
            bad.append((name, dn, dc, allow))
    print("level %s: largest native distance / allowance %.3f" % (ver, worst))
    assert not bad, bad
    heads = ["depth_head"] if ver == "v1" else ["depth_c3", "depth_c4", "fusion"]
    for h in heads:
        a, c = mn.depth_net.get_submodule(h)[1], mc.depth_net.get_submodule(h)[1]
        conv = mn.depth_net.get_submodule(h)[0]
        assert int(a.num_batches_tracked) == int(c.num_batches_tracked) == 1, h
        gap = float((a.running_mean - c.running_mean).abs().max())
        missing = 0.1 * float(conv.bias.abs().max())
        print("running_mean %-12s native vs composition %.3e (a missing m b term: %.3e)" % (h, gap, missing))
        assert gap <= 0.1 * missing, (h, gap, missing)
        assert float((a.running_var - c.running_var).abs().max()) <= 2.0 ** -7 * float(c.running_var.abs().max()), h


def test_level_fp32_tail_native_vs_fp64_yardstick(golden, monkeypatch, report):
    """v2 in train mode without autocast: the 3x3 units stay on torch (composition counter), the tail is
    `_DepthFuseFn` - F.interpolate patched to raise, F.batch_norm patched to raise for the fusion BatchNorm's 41
    channels (the heads' own nn.BatchNorm2d, 256 channels, still go through it).  Against the fp64 yardstick of
    test_vovnet_lift_grad_gpu.py under that file's rule: dev <= max(1, 2 x the composition's dev), the zero-gradient
    biases at its `zero_grad_names` bound."""
    m, c3, c4, calib, G = _small(golden, "v2")
    G = G.cpu()
    ref, _ = TL.yardstick(m, c3, c4, calib, G)
    state = copy.deepcopy(m.state_dict())
    comp = TL.run_level(m, c3, c4, calib, G, native=False)
    m.load_state_dict(state)
    monkeypatch.setenv("LSS_DEPTH_TAIL_NATIVE", "1")
    monkeypatch.setattr(torch.nn.functional, "interpolate", _raiser("interpolate"))
    real_bn = torch.nn.functional.batch_norm

    def batch_norm(x, *a, **k):
        if x.shape[1] == 41:
            raise AssertionError("torch.nn.functional.batch_norm called for the fusion BatchNorm")
        return real_bn(x, *a, **k)

    monkeypatch.setattr(torch.nn.functional, "batch_norm", batch_norm)
    before = _calls()
    nat = TL.run_level(m, c3, c4, calib, G, native=True)
    assert _moved(before) == {"heads": (0, 2), "tail": (1, 0), "lift": (1, 0)}
    zeros = TL.zero_grad_names(m, "v2")
    bad = []
    for k in sorted(ref):
        if k in zeros:
            lim = 2e-5 * float(ref[zeros[k]].abs().max())
            zn = float(nat[k].abs().max()) / lim
            print("fp32 v2 %-40s zero gradient: |g| / bound native %.4f" % (k, zn))
            if not zn <= 1.0:
                bad.append((k, zn, 1.0))
            continue
        dc, dn = TL.dev(comp[k], ref[k]), TL.dev(nat[k], ref[k])
        print("fp32 v2 %-40s dev composition %.4f native %.4f" % (k, dc, dn))
        report("depth_heads.fp32_v2.%s.native" % k, dn)
        bound = 1.0 if k in TL.direct_names("v2") else max(1.0, 2.0 * dc)
        if not dn <= bound:
            bad.append((k, dn, bound))
    assert not bad, bad
    assert int(torch.count_nonzero(nat["depth_net.fusion.0.bias"])) == 0


FALLBACKS = {
    # case: (autocast dtype, expected moves of (heads, tail) as (native, composition))
    "heads_switch_off": (torch.bfloat16, (0, 2), (1, 0)),
    "tail_switch_off": (torch.bfloat16, (2, 0), (0, 1)),
    "eval_batchnorm_in_a_head": (torch.bfloat16, (1, 1), (1, 0)),
    "eval_batchnorm_in_fusion": (torch.bfloat16, (2, 0), (0, 1)),
    "fp16_autocast": (torch.float16, (0, 2), (1, 0)),
    "sync_marker_on_fusion": (torch.bfloat16, (2, 0), (0, 1)),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_fallbacks_advance_only_the_expected_counter(golden, monkeypatch, case):
    """Each switch off, an eval-mode BatchNorm in a head and in `fusion`, fp16 autocast (the units are bf16 only; the
    tail's math is fp32 either way) and an `_lss_sync` marker on the fusion BatchNorm: the counters move as listed and
    every gradient is finite."""
    amp, heads, tail = FALLBACKS[case]
    m, c3, c4, calib, G = _small(golden, "v2")
    monkeypatch.setenv("LSS_DEPTH_HEADS_NATIVE", "0" if case == "heads_switch_off" else "1")
    monkeypatch.setenv("LSS_DEPTH_TAIL_NATIVE", "0" if case == "tail_switch_off" else "1")
    if case == "eval_batchnorm_in_a_head":
        m.depth_net.depth_c4[1].eval()
    if case == "eval_batchnorm_in_fusion":
        m.depth_net.fusion[1].eval()
    if case == "sync_marker_on_fusion":
        m.depth_net.fusion[1].__dict__["_lss_sync"] = (None,)
    before = _calls()
    out = _level_step(m, c3, c4, calib, G, amp)
    assert _moved(before) == {"heads": heads, "tail": tail, "lift": (1, 0)}
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_capture_train_level_replays_equal_eager(golden, monkeypatch, ver):
    """The train-mode level under bf16 autocast with both routes native - no library convolution in it, conv2d is
    patched to raise throughout - captured in one graph after three eager warm-up steps and replayed three times on
    refreshed static inputs: bev and every gradient equal the eager step's bit for bit on every replay."""
    from lss2_multimodal_nu_amd.data import prepare_calibration
    monkeypatch.setenv("LSS_DEPTH_HEADS_NATIVE", "1")
    monkeypatch.setenv("LSS_DEPTH_TAIL_NATIVE", "1")
    m, c3, c4, calib, G = _small(golden, ver)
    pack = prepare_calibration(*calib, pin=True)
    c3, c4 = c3.cuda().requires_grad_(True), c4.cuda().requires_grad_(True)
    leaves = [c3] + ([c4] if ver == "v2" else []) + [p for _, p in TL.level_params(m)]
    monkeypatch.setattr(torch.nn.functional, "conv2d", _raiser("conv2d"))

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            bev = m.get_voxels(c3, c4, pack, None, None, None, None)
        return (bev,) + torch.autograd.grad((bev.float() * G).sum(), leaves)

    before = _calls()
    TL._capture_and_replay(step, (c3, c4))
    units, tails = (1, 0) if ver == "v1" else (2, 1)
    assert _moved(before) == {"heads": (7 * units, 0), "tail": (7 * tails, 0), "lift": (7, 0)}
