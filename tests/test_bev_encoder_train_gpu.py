"""The native training route of `BEVEncoderTransformer` (bf16 autocast): the 64-channel head kernels, the biased 3x3
unit, the 1x1 `compress` unit, and the module - route, fallbacks, `forward_loss`, graph capture.

References, bounds and cases: tests/bev_encoder_train_ref.py (held against torch's fp64 autograd by
tests/test_bev_encoder_train_ref_cpu.py).  Every measured error is printed and `report`ed before it is asserted."""
import copy

import pytest
import torch
from torch import nn
from torch.nn import functional as F

import bev_encoder_train_ref as E
import train_node_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402
from lss2_multimodal_nu_amd import modules as M  # noqa: E402
from lss2_multimodal_nu_amd import ops, tools  # noqa: E402
from lss2_multimodal_nu_amd import transformer_modules as tm  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------
# 1. the head over 64-channel rows
# ---------------------------------------------------------------------------------------------------------------------
def _head_gpu(op):
    y = op["y"].to(torch.bfloat16).cuda()
    w, b, cw = op["w"].cuda(), op["b"].cuda(), op["cw"].cuda()
    t, g = op["t"].cuda(), op["g"].cuda()
    loss, sums = ops.head_ce_fwd(y, w, b, t, cw)
    dy, dw, db = ops.head_ce_bwd(y, w, b, t, cw, sums, torch.tensor(op["gl"]).cuda())
    logits = ops.head1x1_fwd(y, w, b)
    hdy, hdw, hdb = ops.head1x1_bwd(y, w, b, g)
    torch.cuda.synchronize()
    return {"logits": logits, "loss": loss, "ce_dy": dy, "ce_dw": dw, "ce_db": db, "h_dy": hdy, "h_dw": hdw, "h_db": hdb}


@pytest.mark.parametrize("case", E.HEAD_CASES, ids=lambda c: c[0])
def test_head_64_channels_all_four_modes_vs_fp64(case, report):
    """head_ce_kernel with CIN = 64 (8 lanes per pixel, 8 pixels per wave pass): fused head + weighted cross-entropy
    forward / backward and the head alone forward / backward against the fp64 reference on the same bf16 rows, at the
    bounds of the 128-channel tests; a repeated call reproduces every output bit for bit.  Shapes: a ragged last wave
    pass (70 pixels), a second trip of the grid-stride loop (17 408 pixels), ignored targets and a zero-weight class.
    Measured (MI355X), largest over the cases: logits 1.5e-7, loss 9.1e-8, dy 3.6e-3 (bound 3.9e-3), dW / db 1.9e-7."""
    op = E.make_head_operands(*case)
    ref = E.head_evaluate(op)
    got = _head_gpu(op)
    assert got["logits"].dtype == torch.float32 and got["ce_dy"].dtype == got["h_dy"].dtype == torch.bfloat16
    bad = []
    for key, err in sorted(E.head_errors(got, ref).items()):
        print("head %-34s %-7s %.3e (bound %.1e)" % (case[0], key, err, E.head_bound(key)))
        report("bev_encoder.head.%s.%s" % (case[0], key), err)
        if not err <= E.head_bound(key):
            bad.append((key, err))
    assert not bad, bad
    again = _head_gpu(op)
    for key in got:
        assert torch.equal(got[key], again[key]), key


def test_tools_head_functions_take_64_channels():
    """tools.head_1x1 / head_weighted_cross_entropy route a bf16 64-channel activation to the native nodes."""
    op = E.make_head_operands(*E.HEAD_CASES[0])
    head = nn.Conv2d(64, 4, 1).cuda()
    y = op["y"].to(torch.bfloat16).cuda().permute(0, 3, 1, 2).requires_grad_(True)
    out = tools.head_1x1(y, head)
    assert type(out.grad_fn).__name__ == "_Head1x1FnBackward" and out.dtype == torch.float32
    loss = tools.head_weighted_cross_entropy(y, head, op["t"].cuda(), op["cw"].cuda())
    assert type(loss.grad_fn).__name__ == "_HeadCEFnBackward"
    want = tools.weighted_cross_entropy(out, op["t"].cuda(), op["cw"].cuda())
    assert abs(float(loss.detach()) - float(want.detach())) <= 2e-5 * abs(float(want.detach()))


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 4. the units
# ---------------------------------------------------------------------------------------------------------------------
FUSED_TAGS = {"conv_bn_act_train_fwd", "conv_bn_act_train_bwd"}
UNIT_1X1_TAGS = {"linear", "linear_dgrad", "linear_wgrad", "bn_train_fwd", "bn_train_bwd"}


def _unit_modules(op):
    Co, Ct, k, _ = op["w"].shape
    conv = nn.Conv2d(Ct, Co, k, padding=op["pad"], bias=True).cuda()
    bn = nn.BatchNorm2d(Co, eps=R.EPS, momentum=R.MOMENTUM).cuda().train()
    with torch.no_grad():
        conv.weight.copy_(op["w"])
        conv.bias.copy_(op["bias"])
        bn.weight.copy_(op["gamma"])
        bn.bias.copy_(op["beta"])
        bn.running_mean.copy_(op["running_mean"])
        bn.running_var.copy_(op["running_var"])
    return conv, bn


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).double().cpu()


def _run_unit(op):
    """One forward + backward of the biased unit under bf16 autocast.  Returns (outputs as fp64 CPU tensors under the
    reference's names, timer tags, the exact bias gradient tensor, num_batches_tracked)."""
    conv, bn = _unit_modules(op)
    k = op["w"].shape[2]
    x1 = op["x1"].cuda().to(torch.bfloat16).requires_grad_(True)
    timer = ops.KernelTimer(fine=True)
    ops.set_timer(timer)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if k == 3:
                y = M._train_conv_bn_act(conv, bn, x1, True)
            else:
                assert M._conv1x1_unit_ok(conv, bn, x1)
                y = M._train_conv1x1_bn_act(conv, bn, x1)
        assert type(y.grad_fn).__name__ == "_AbsorbedBiasFnBackward", type(y.grad_fn).__name__
        node = y.grad_fn.next_functions[0][0]
        saved = node.saved_tensors
        got = {"y": y.detach().double().cpu()}
        if k == 3:   # x1n, x2n, z, y, w, gamma, stat = (mean, invstd)
            assert type(node).__name__ == "_ConvBNActFnBackward" and len(saved) == 7
            got.update(z=_nchw(saved[2]), mean=saved[6][0].double().cpu(), invstd=saved[6][1].double().cpu())
        else:        # zn, y, gamma, mean, invstd
            assert type(node).__name__ == "_BNActFnBackward" and len(saved) == 5
            got.update(z=_nchw(saved[0]), mean=saved[3].double().cpu(), invstd=saved[4].double().cpu())
        leaves = {"g1": x1, "dw": conv.weight, "dbias": conv.bias, "dgamma": bn.weight, "dbeta": bn.bias}
        grads = torch.autograd.grad(y, list(leaves.values()), op["gy"].cuda().to(torch.bfloat16))
        torch.cuda.synchronize()
    finally:
        ops.set_timer(None)
    got.update({k_: g.detach().double().cpu() for k_, g in zip(leaves, grads)})
    got.update(running_mean=bn.running_mean.double().cpu(), running_var=bn.running_var.double().cpu())
    return got, set(timer.spans), grads[2], int(bn.num_batches_tracked)


def _assert_unit(report, name, got, op):
    """Mask check, fp64 reference with the unit's own mask, floor, FACTOR x floor for every output."""
    R.mask_check(got["y"], E.unit_reference(op))
    mask = (got["y"] > 0).double()
    ref, emu = E.unit_reference(op, mask), E.unit_evaluate(op, mask, emulate=True)
    floor = R.floors(ref, emu, E.UNIT_OUTPUTS)
    bound = R.bounds(floor)
    bad = []
    for key in E.UNIT_OUTPUTS:
        e = R.errors(got[key], ref[key])
        print("unit %-32s %-13s max %.3e l2 %.3e (floor %.3e %.3e)" % ((name, key) + e + floor[key]))
        for metric, ev, bv in zip(("max", "l2"), e, bound[key]):
            report("bev_encoder.unit.%s.%s.%s" % (name, key, metric), ev)
            if not ev <= bv:
                bad.append("%s %s: %.3e > %.3e" % (key, metric, ev, bv))
    assert not bad, (name, bad)


def _assert_bias_rule(bias_grad, op, batches):
    assert bias_grad.dtype == torch.float32 and tuple(bias_grad.shape) == tuple(op["bias"].shape)
    assert int(torch.count_nonzero(bias_grad)) == 0, "conv.bias.grad must be a tensor of exact zeros"
    assert batches == 1


@pytest.mark.parametrize("u", E.BIASED_3X3, ids=lambda u: u.name)
def test_biased_3x3_unit_vs_fp64(u, report):
    """`_train_conv_bn_act` with nn.Conv2d(bias=True) in front of a train-mode BatchNorm: the fused bias-free node
    (spans conv_bn_act_train_fwd / _bwd), y, dx, dW, dgamma, dbeta and both running statistics within FACTOR x the
    rounding floor of the fp64 reference of the BIASED unit, conv.bias.grad a tensor of exact zeros,
    num_batches_tracked advanced by one."""
    op = E.make_unit_operands(u)
    ops.prepack.clear()
    got, tags, bias_grad, batches = _run_unit(op)
    assert FUSED_TAGS <= tags, tags
    _assert_bias_rule(bias_grad, op, batches)
    _assert_unit(report, u.name, got, op)
    ops.assert_no_timeouts(u.name)


def test_biased_3x3_unit_ring_shape_against_the_tile_kernels(monkeypatch, report):
    """2 x 96 x 160, 256 -> 128: the forward conv takes the ring kernel (asserted).  The same unit with
    LSS_CONV_RING=0 in the same process is within the bound of the same widths' small case (there is no fp64 conv of
    this size: the floor per output depends on the channel counts and the storage roundings, not on the extent)."""
    u = E.RING
    assert ops.N.lib().lss_conv2d_ring_ok(2, 96, 160, 256, 0, 1, 128, 0) == 1
    op = E.make_unit_operands(u)
    ops.prepack.clear()
    ring, tags, bias_grad, batches = _run_unit(op)
    assert FUSED_TAGS <= tags
    _assert_bias_rule(bias_grad, op, batches)
    monkeypatch.setenv("LSS_CONV_RING", "0")
    assert not ops.conv_ring_ok(2, 96, 160, 256, 0, 1, 128, 0)
    ops.prepack.clear()
    tile, _, _, _ = _run_unit(op)
    ops.prepack.clear()
    small = E.make_unit_operands(next(s for s in E.BIASED_3X3 if s.name == E.RING_FLOOR_FROM))
    mask = (E.unit_reference(small)["t"] > 0).double()
    bound = R.bounds(R.floors(E.unit_reference(small, mask), E.unit_evaluate(small, mask, emulate=True), E.UNIT_OUTPUTS))
    bad = []
    for key in E.UNIT_OUTPUTS:
        e = R.errors(ring[key], tile[key])
        print("ring vs tile %-13s max %.3e l2 %.3e (bound %.3e %.3e)" % ((key,) + e + bound[key]))
        report("bev_encoder.ring_ab.%s.max" % key, e[0])
        if not (e[0] <= bound[key][0] and e[1] <= bound[key][1]):
            bad.append((key, e, bound[key]))
    assert not bad, bad
    ops.assert_no_timeouts(u.name)


@pytest.mark.parametrize("u", E.CONV_1X1, ids=lambda u: u.name)
def test_conv1x1_unit_vs_fp64(u, report):
    """`_train_conv1x1_bn_act` (the `compress` unit): the GEMM node of the transformer's linears + `_BNActFn` with the
    bias rule, same quantities and bounds as the 3x3 unit."""
    op = E.make_unit_operands(u, ksize=1)
    got, tags, bias_grad, batches = _run_unit(op)
    assert UNIT_1X1_TAGS <= tags and not (FUSED_TAGS & tags), tags
    _assert_bias_rule(bias_grad, op, batches)
    _assert_unit(report, u.name, got, op)


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 8. the module
# ---------------------------------------------------------------------------------------------------------------------
def _module(cin=64, K=4, seed=5):
    torch.manual_seed(0)
    m = mv.BEVEncoderTransformer(cin, K)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, tm.DeformableAttention):
                mod.sampling_offsets.weight.copy_(torch.randn(mod.sampling_offsets.weight.shape, generator=g) * 0.05)
                mod.attention_weights.weight.copy_(torch.randn(mod.attention_weights.weight.shape, generator=g) * 0.05)
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
            if isinstance(mod, nn.Conv2d):   # biases of the order of the activations, not the default 1 / sqrt(fan_in)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.5)
    return m.cuda().train()


def _inputs(cin=64, K=4, B=2, H=24, seed=6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, H, generator=g).cuda()
    target = (torch.rand(B, K, H, H, generator=g) > 0.7).float().cuda()
    labels = torch.randint(0, K, (B, H, H), generator=g).cuda()
    return x, target, labels


def _bce_step(m, x, target, autocast):
    """Loss and every parameter gradient of one BCE step; autocast: None (fp32) or a dtype."""
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        seg, refined = m(x)
        loss = F.binary_cross_entropy_with_logits(seg.float(), target)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), seg, refined, {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _calls():
    return dict(mv.BEV_ENCODER_CALLS)


def _moved(before):
    return {k: mv.BEV_ENCODER_CALLS[k] - before[k] for k in before}


PRE_BN_BIASES = ("compress.0.bias", "seg_head.0.bias", "seg_head.3.bias")


def _no_conv2d(*a, **k):
    raise AssertionError("torch.nn.functional.conv2d called on the native route")


def test_module_native_against_composition_through_fp32(monkeypatch, report):
    """BEVEncoderTransformer(64, 4) on 2 x 64 x 24 x 24, dropout 0, BatchNorms in training mode, BCE loss; three runs
    from the same state: fp32 without autocast (the middle), the bf16 composition (LSS_BEV_ENCODER_NATIVE=0) and the
    bf16 native route with torch.nn.functional.conv2d patched to raise.  For the loss and every parameter gradient,
    max |native - middle| <= 2 max |composition - middle| + 2^-9 max |middle|.  The three biases in front of a BatchNorm
    are left out (their exact gradient is zero: both bf16 paths and fp32 hold rounding noise or nothing) and asserted
    to be exact zeros on the native route.
    Measured (MI355X), max distance to the fp32 middle relative to the middle's largest element, composition / native
    (the train-mode BatchNorm backwards amplify bf16 rounding for both paths alike):
      compress.0.weight 1.26e-1 / 1.38e-1     compress.1.weight 1.05e-1 / 1.29e-1, .bias 1.18e-1 / 1.08e-1
      seg_head.0.weight 1.57e-1 / 1.45e-1     seg_head.1.weight 6.71e-2 / 1.08e-1, .bias 1.88e-1 / 1.74e-1
      seg_head.3.weight 1.64e-1 / 1.55e-1     seg_head.4.weight 2.96e-3 / 1.68e-3, .bias 1.46e-2 / 1.65e-2
      seg_head.6.weight 6.38e-3 / 2.59e-3, .bias 1.13e-3 / 8.77e-5
      transformer: sampling_offsets.weight 1.37e-1 / 2.02e-1 (the largest native figure), value_proj.weight
      1.01e-1 / 9.86e-2, norm1.weight 9.35e-2 / 1.12e-1, norm2.weight 8.59e-2 / 1.08e-1
    largest native distance / allowance over all tensors: 0.79 (seg_head.1.weight)."""
    m0 = _module()
    x, target, _ = _inputs()
    mid = _bce_step(copy.deepcopy(m0), x, target, None)
    monkeypatch.setenv("LSS_BEV_ENCODER_NATIVE", "0")
    before = _calls()
    comp = _bce_step(copy.deepcopy(m0), x, target, torch.bfloat16)
    assert _moved(before) == {"native": 0, "composition": 1}
    monkeypatch.delenv("LSS_BEV_ENCODER_NATIVE")
    monkeypatch.setattr(torch.nn.functional, "conv2d", _no_conv2d)
    before = _calls()
    mn = copy.deepcopy(m0)
    nat = _bce_step(mn, x, target, torch.bfloat16)
    assert _moved(before) == {"native": 1, "composition": 0}
    assert nat[1].dtype == torch.float32 and tuple(nat[1].shape) == (2, 4, 24, 24)
    assert nat[2].dtype == comp[2].dtype and tuple(nat[2].shape) == (2, 256, 24, 24)
    for bn in (mn.compress[1], mn.seg_head[1], mn.seg_head[4]):
        assert int(bn.num_batches_tracked) == 1
    bad, worst = [], 0.0
    rows = [("loss", nat[0], comp[0], mid[0])] + [(n, nat[3][n], comp[3][n], mid[3][n]) for n in sorted(mid[3])]
    for name, a, c, r in rows:
        if name in PRE_BN_BIASES:
            assert int(torch.count_nonzero(a)) == 0, name
            continue
        ok, dn, dc, allow = E.module_within(a, c, r)
        scale = float(r.abs().max())
        print("module %-48s composition %.3e native %.3e" % (name, dc / scale, dn / scale))
        report("bev_encoder.module.%s.native" % name, dn / scale)
        report("bev_encoder.module.%s.composition" % name, dc / scale)
        worst = max(worst, dn / allow)
        if not ok:
            bad.append((name, dn, dc, allow))
    print("module: largest native distance / allowance %.3f" % worst)
    assert not bad, bad


def test_module_running_mean_carries_the_bias(monkeypatch):
    """After one native step the compress BatchNorm's running_mean is what nn.BatchNorm2d holds after the composition's
    step (bf16 noise apart): the m * b term is there.  Without it the two would differ by 0.1 |b|, |b| ~ 0.5."""
    m0 = _module()
    x, target, _ = _inputs()
    mc, mn = copy.deepcopy(m0), copy.deepcopy(m0)
    monkeypatch.setenv("LSS_BEV_ENCODER_NATIVE", "0")
    _bce_step(mc, x, target, torch.bfloat16)
    monkeypatch.delenv("LSS_BEV_ENCODER_NATIVE")
    _bce_step(mn, x, target, torch.bfloat16)
    for name in ("compress.1", "seg_head.1", "seg_head.4"):
        a, c = mn.get_submodule(name), mc.get_submodule(name)
        conv = mn.get_submodule(name[:-1] + str(int(name[-1]) - 1))
        gap = float((a.running_mean - c.running_mean).abs().max())
        missing = 0.1 * float(conv.bias.abs().max())
        print("running_mean %-12s native vs composition %.3e (a missing m b term: %.3e)" % (name, gap, missing))
        assert gap <= 0.1 * missing, (name, gap, missing)
        assert float((a.running_var - c.running_var).abs().max()) <= 2.0 ** -7 * float(c.running_var.abs().max())


@pytest.mark.parametrize("case", ["fp32", "fp16", "switch_off", "eval_batchnorm", "cin_96"])
def test_fallbacks_take_the_composition(case, monkeypatch):
    """fp32, fp16 autocast, LSS_BEV_ENCODER_NATIVE=0, an eval-mode BatchNorm in the seg head and C_in = 96 each advance
    `composition` only and return finite gradients."""
    cin = 96 if case == "cin_96" else 64
    m = _module(cin)
    x, target, _ = _inputs(cin)
    if case == "switch_off":
        monkeypatch.setenv("LSS_BEV_ENCODER_NATIVE", "0")
    if case == "eval_batchnorm":
        m.seg_head[1].eval()
    autocast = {"fp32": None, "fp16": torch.float16}.get(case, torch.bfloat16)
    before = _calls()
    loss, _, _, grads = _bce_step(m, x, target, autocast)
    assert _moved(before) == {"native": 0, "composition": 1}
    assert torch.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())


def test_forward_loss_equals_forward_plus_weighted_cross_entropy(report):
    """`forward_loss(x, target, class_weight)` against `forward` + tools.weighted_cross_entropy on the same weights
    under bf16 autocast (both on the native route): the loss within 2e-5 relative, every gradient under the rule of the
    module test with the fp32 two-step form as the middle and the bf16 two-step form as the yardstick."""
    m0 = _module()
    x, _, labels = _inputs()
    cw = torch.tensor([1.0, 10.0, 5.0, 10.0]).cuda()

    def two_step(m, autocast):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            seg, _ = m(x)
            loss = tools.weighted_cross_entropy(seg.float(), labels, cw)
        loss.backward()
        return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    mid = two_step(copy.deepcopy(m0), False)
    before = _calls()
    two = two_step(copy.deepcopy(m0), True)
    mf = copy.deepcopy(m0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, refined = mf.forward_loss(x, labels, cw)
    assert type(loss.grad_fn).__name__ == "_HeadCEFnBackward" and tuple(refined.shape) == (2, 256, 24, 24)
    loss.backward()
    torch.cuda.synchronize()
    assert _moved(before) == {"native": 2, "composition": 0}
    err = abs(float(loss) - float(two[0])) / abs(float(two[0]))
    print("forward_loss vs forward + weighted_cross_entropy: relative loss difference %.3e" % err)
    assert report("bev_encoder.forward_loss.loss", err) <= 2e-5
    bad = []
    for n, p in mf.named_parameters():
        if n in PRE_BN_BIASES:
            assert int(torch.count_nonzero(p.grad)) == 0, n
            continue
        ok, dn, dc, allow = E.module_within(p.grad, two[1][n], mid[1][n])
        if not ok:
            bad.append((n, dn, dc, allow))
    assert not bad, bad


def _capture_and_replay(step, statics, state):
    """Warm up on a side stream, capture one step, replay three times on refreshed static inputs; after every replay
    the same step runs eagerly from the same `state` (tensors the step updates in place) and must give the same bits."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    gen = torch.Generator().manual_seed(12)
    for r in range(3):
        with torch.no_grad():
            for s_ in statics:
                s_.copy_(torch.randn(s_.shape, generator=gen))
        start = [s_.clone() for s_ in state]
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static_out] + [s_.clone() for s_ in state]
        with torch.no_grad():
            for s_, v in zip(state, start):
                s_.copy_(v)
        want = list(step())
        torch.cuda.synchronize()
        want += [s_.clone() for s_ in state]
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (r, i)


def test_capture_forward_backward_replays_equal_eager():
    """Forward + backward of the module (dropout 0) on the native route captured in one `torch.cuda.graph` after three
    eager warm-up steps on a side stream and replayed three times on refreshed static inputs: the loss, every
    gradient and both running statistics of the three BatchNorms equal the eager step's bit for bit."""
    m = _module()
    x, target, _ = _inputs()
    x.requires_grad_(True)
    params = [p for _, p in m.named_parameters()]
    state = []
    for bn in (m.compress[1], m.seg_head[1], m.seg_head[4]):
        state += [bn.running_mean, bn.running_var, bn.num_batches_tracked]

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            seg, _ = m(x)
            loss = F.binary_cross_entropy_with_logits(seg.float(), target)
        return (loss.detach(),) + torch.autograd.grad(loss, [x] + params)

    before = _calls()
    _capture_and_replay(step, (x,), state)
    assert _moved(before) == {"native": 3 + 1 + 3, "composition": 0}
