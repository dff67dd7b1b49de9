"""The training route of the vovnet camera branch on the GPU: K16's weight and bias gradients alone against fp64, the
tap-list conv-BN node against the fp64 reference under the 3 x floor rule (tests/tapconv_train_ref.py), and the branch
on the model at production widths: no further from an fp32 run than twice torch's own bf16 autocast composition, with
no library convolution, reproducible under dropout, capturable, and routed as documented.  Every measured error is
`report`ed."""
import copy
import gc

import numpy as np
import pytest
import torch

import tapconv_train_ref as R

pytestmark = pytest.mark.gpu

import lss2_multimodal_nu_amd as L  # noqa: E402
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402
from lss2_multimodal_nu_amd import modules, ops  # noqa: E402
from oracle import vovnet_oracle as vo  # noqa: E402

GRID_COARSE = dict(xbound=[-50.0, 50.0, 2.0], ybound=[-50.0, 50.0, 2.0], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
BF16 = dict(device_type="cuda", dtype=torch.bfloat16)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_and_bias_grad_against_fp64(case, report):
    """bf16 operands in, fp32 out, nothing rounded in between: the rounding floor is 0 and the bound is the fp32 minimum
    of the convention, 2e-4 in both metrics (fp32 accumulation over at most 3 x 176 exact products is ~1e-6)."""
    BN, H, W, Cin, Cout, k, d = case
    tag = "tapconv_train.wgrad.%s." % "x".join(map(str, case))
    x, dy = R.make_wgrad_operands(case)
    xn, dyn = _nhwc(x), _nhwc(dy)
    assert ops.tapconv_wgrad_ok(BN, H, W, Cin, Cout)
    dw = ops.tapconv_wgrad(xn, dyn, k, d)
    assert dw.shape == (Cout, Cin, k, k) and dw.dtype == torch.float32
    ref = R.wgrad_reference(x, dy, k, d)
    emax, el2 = R.errors(dw, ref)
    report(tag + "max", emax)
    report(tag + "l2", el2)
    print("%s max %.3e l2 %.3e" % (tag, emax, el2))
    assert emax <= R.T.MIN_F32 and el2 <= R.T.MIN_F32
    dead = sorted(set(range(k * k)) - set(R.live_taps(H, W, k, d)))
    assert len(dead) == k * k - len(ops.live_taps(H, W, k, d))
    if dead:
        assert int(torch.count_nonzero(dw.view(Cout, Cin, k * k)[:, :, dead])) == 0   # exactly 0, not small
    assert torch.equal(ops.tapconv_wgrad(xn, dyn, k, d), dw)                          # bit-identical run to run
    assert int(torch.count_nonzero(ops.tapconv_wgrad(xn, torch.zeros_like(dyn), k, d))) == 0
    db = ops.tapconv_bias_grad(dyn)
    assert db.shape == (BN, Cout) and db.dtype == torch.float32
    emax, el2 = R.errors(db, dy.double().sum((2, 3)))
    report(tag + "bias.max", emax)
    assert emax <= R.T.MIN_F32 and el2 <= R.T.MIN_F32
    assert torch.equal(ops.tapconv_bias_grad(dyn), db)


# ---------------------------------------------------------------------------------------------------------------------
# the node
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u", R.UNITS, ids=lambda u: u.name)
def test_node_against_reference(u, report):
    op = R.make_operands(u)
    conv = torch.nn.Conv2d(u.Cin, u.Cout, u.k, padding=u.d if u.k == 3 else 0, dilation=u.d, bias=u.conv_bias).cuda()
    bn = torch.nn.BatchNorm2d(u.Cout, eps=R.EPS, momentum=R.MOMENTUM).cuda()
    with torch.no_grad():
        conv.weight.copy_(op["w"])
        if u.conv_bias:
            conv.bias.copy_(op["b"])
        bn.weight.copy_(op["gamma"])
        bn.bias.copy_(op["beta"])
        bn.running_mean.copy_(op["running_mean"])
        bn.running_var.copy_(op["running_var"])
    x = op["x"].cuda().requires_grad_(True)
    ib = None if op["img_bias"] is None else op["img_bias"].cuda().requires_grad_(True)
    with torch.autocast(**BF16):
        assert modules._tapconv_unit_ok(conv, bn, x)
        y = modules._train_tapconv_bn_act(conv, bn, x, relu=u.relu, img_bias=ib)
    assert y.shape == (u.BN, u.Cout, u.H, u.W) and y.dtype == torch.bfloat16
    leaves = {"g1": x, "dw": conv.weight, "dgamma": bn.weight, "dbeta": bn.bias, "dbias": ib, "db": conv.bias}
    keys = [k for k, v in leaves.items() if v is not None]
    got = dict(zip(keys, torch.autograd.grad(y, [leaves[k] for k in keys], op["gy"].cuda().to(y.dtype))))
    got.update(y=y.detach().float(), running_mean=bn.running_mean, running_var=bn.running_var)
    assert got["dw"].dtype == torch.float32 and got["g1"].dtype == torch.float32
    assert int(bn.num_batches_tracked) == 1                           # as nn.BatchNorm2d counts

    mask = (y.detach().cpu() > 0) if u.relu else None
    ref = R.reference(op, mask)
    if u.relu:
        frac, flips = R.mask_check(y, ref)
        report("tapconv_train.node.%s.band" % u.name, frac)
    bound = R.bounds(R.floors(ref, R.evaluate(op, mask, emulate=True)))
    for k in ("y", "g1", "dw", "dgamma", "dbeta", "running_mean", "running_var") + (("dbias",) if u.img_bias else ()):
        emax, el2 = R.errors(got[k], ref[k])
        report("tapconv_train.node.%s.%s.max" % (u.name, k), emax)
        print("node %-18s %-13s max %.3e (bound %.3e) l2 %.3e (bound %.3e)" % (u.name, k, emax, bound[k][0], el2, bound[k][1]))
        assert emax <= bound[k][0] and el2 <= bound[k][1], (k, emax, el2, bound[k])
    if u.conv_bias:
        assert got["db"].shape == conv.bias.shape and int(torch.count_nonzero(got["db"])) == 0
        # running_mean includes momentum * b: without it the error would be about |b| momentum / |running_mean| ~ 0.3
        bare = R.errors(bn.running_mean - R.MOMENTUM * conv.bias.detach(), ref["running_mean"])[0]
        assert bare > 10 * bound["running_mean"][0]
    dead = sorted(set(range(u.k ** 2)) - set(R.live_taps(u.H, u.W, u.k, u.d)))
    if dead:
        assert int(torch.count_nonzero(got["dw"].view(u.Cout, u.Cin, -1)[:, :, dead])) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the branch on the model
# ---------------------------------------------------------------------------------------------------------------------
TAIL = ("feature_pyramid", "sceneunder")


class _Trunk(mv.TrunkC3C4):
    def __init__(self, c3, c4):
        super().__init__()
        self.c3_channels, self.c4_channels = c3, c4


def _state_shapes(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


@pytest.fixture(scope="module")
def model():
    """Production widths (768-channel c3, six cameras, 8 x 22 maps), B = 1, seeded TXT-branch parameters, training mode,
    the projection's dropout off unless a test turns it on."""
    conf = dict(final_dim=(128, 352), Ncams=6, cams=list("abcdef"))
    torch.manual_seed(40)
    m = L.compile_model_vovnet_transformer(1, GRID_COARSE, conf, 4, lss_version="v2", precision="bf16")
    for i, n in enumerate(TAIL):
        sub = getattr(m, n)
        sub.load_state_dict(vo.seeded_state(_state_shapes(sub), 40 + i))
    m = m.cuda().train()
    m.sceneunder[0].project[3].p = 0.0
    yield m
    del m
    gc.collect()
    torch.cuda.empty_cache()


def _branch_params(m):
    return [(n + "." + k, p) for n in TAIL for k, p in getattr(m, n).named_parameters()]


def _c3(seed, BN=6, cin=768, H=8, W=22):
    return torch.from_numpy(np.random.RandomState(seed).randn(BN, cin, H, W).astype(np.float32)).cuda()


def _token_weights():
    return torch.from_numpy(np.random.RandomState(77).randn(6, 256).astype(np.float32)).cuda()


def _step(m, c3_values, autocast, state=None):
    """One forward + backward of `scene_tokens` from `state`: {name: tensor} of tokens, c3.grad and parameter grads."""
    if state is not None:
        for n in TAIL:
            getattr(m, n).load_state_dict(state[n])
    for _, p in _branch_params(m):
        p.grad = None
    c3 = c3_values.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=autocast or torch.bfloat16, enabled=autocast is not None):
        tok = m.scene_tokens(c3)
    assert tok.shape == (6, 256)      # fp32 on the native route; the library composition under autocast returns bf16
    (tok.float() * _token_weights()).sum().backward()
    out = {"tokens": tok.detach().clone(), "c3.grad": c3.grad.clone()}
    for n, p in _branch_params(m):
        assert p.grad is not None, n
        out[n] = p.grad.detach().clone().float()
    return out


def _raise_conv(*a, **k):
    raise AssertionError("a library convolution ran on the native training route")


def test_branch_against_fp32_and_the_autocast_composition(model, monkeypatch, report):
    m = model
    state = {n: copy.deepcopy(getattr(m, n).state_dict()) for n in TAIL}
    c3 = _c3(5)
    before = dict(mv.CAMERA_BRANCH_TRAIN_CALLS)
    fp32 = _step(m, c3, None, state)
    monkeypatch.setenv("LSS_CAMERA_BRANCH_TRAIN_NATIVE", "0")
    comp = _step(m, c3, torch.bfloat16, state)
    assert mv.CAMERA_BRANCH_TRAIN_CALLS == {"native": before["native"], "composition": before["composition"] + 2}
    monkeypatch.setenv("LSS_CAMERA_BRANCH_TRAIN_NATIVE", "1")
    old = dict(mv.CAMERA_BRANCH_CALLS)
    with monkeypatch.context() as mp:
        mp.setattr(torch.nn.functional, "conv2d", _raise_conv)
        native = _step(m, c3, torch.bfloat16, state)
    assert native["tokens"].dtype == torch.float32
    assert mv.CAMERA_BRANCH_TRAIN_CALLS == {"native": before["native"] + 1, "composition": before["composition"] + 2}
    assert mv.CAMERA_BRANCH_CALLS == old                              # the inference counter does not see the training route
    bns = [b for n in TAIL for b in getattr(m, n).modules() if isinstance(b, torch.nn.BatchNorm2d)]
    assert len(bns) == 9 and all(int(b.num_batches_tracked) == int(state["feature_pyramid"]["scale1.1.num_batches_tracked"]) + 1
                                 for b in bns)
    assert set(native) == set(comp) == set(fp32) and len(native) == 2 + 9 * 3 + 3
    failures = []
    for k in sorted(fp32):
        en, ec = R.errors(native[k], fp32[k]), R.errors(comp[k], fp32[k])
        report("tapconv_train.branch.%s.native.l2" % k, en[1])
        report("tapconv_train.branch.%s.composition.l2" % k, ec[1])
        print("branch %-46s native max %.3e l2 %.3e   composition max %.3e l2 %.3e" % (k, en[0], en[1], ec[0], ec[1]))
        if not (en[0] <= 2 * ec[0] and en[1] <= 2 * ec[1]):
            failures.append((k, en, ec))
    assert not failures, failures


def test_dropout_runs_are_bit_identical(model):
    m = model
    c3 = _c3(6)
    m.sceneunder[0].project[3].p = 0.5
    try:
        before = mv.CAMERA_BRANCH_TRAIN_CALLS["native"]
        runs = []
        for _ in range(2):
            torch.manual_seed(11)
            runs.append(_step(m, c3, torch.bfloat16))
        assert mv.CAMERA_BRANCH_TRAIN_CALLS["native"] == before + 2
        torch.manual_seed(12)
        other = _step(m, c3, torch.bfloat16)
    finally:
        m.sceneunder[0].project[3].p = 0.0
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert not torch.equal(runs[0]["tokens"], other["tokens"])        # the dropout does draw


def test_forward_and_backward_replay_in_a_graph(model):
    """After one eager step (which allocates the cached workspaces and registers the weight packs) forward + backward
    are captured once; every replay gives the eager gradients bit for bit."""
    m = model
    c3v = _c3(7)
    eager = _step(m, c3v, torch.bfloat16)
    params = _branch_params(m)
    c3 = c3v.clone().requires_grad_(True)
    wt = _token_weights()
    for _, p in params:
        p.grad = None
    before = mv.CAMERA_BRANCH_TRAIN_CALLS["native"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with torch.autocast(**BF16):
            tok = m.scene_tokens(c3)
        (tok * wt).sum().backward()
    assert mv.CAMERA_BRANCH_TRAIN_CALLS["native"] == before + 1
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(tok, eager["tokens"]), i
        assert torch.equal(c3.grad, eager["c3.grad"]), i
        for n, p in params:
            assert torch.equal(p.grad.float(), eager[n]), (i, n)
    del g
    for _, p in params:
        p.grad = None


def test_fallbacks_take_the_composition(model, monkeypatch):
    m = model
    c3 = _c3(8)

    def composition(fn):
        before = dict(mv.CAMERA_BRANCH_TRAIN_CALLS)
        fn()
        assert mv.CAMERA_BRANCH_TRAIN_CALLS == {"native": before["native"], "composition": before["composition"] + 1}

    def call(dtype):
        with torch.autocast("cuda", dtype=dtype):
            return m.scene_tokens(c3.clone().requires_grad_(True))

    before = mv.CAMERA_BRANCH_TRAIN_CALLS["native"]
    call(torch.bfloat16)
    assert mv.CAMERA_BRANCH_TRAIN_CALLS["native"] == before + 1       # the route is there to fall back from
    monkeypatch.setenv("LSS_CAMERA_BRANCH_TRAIN_NATIVE", "0")
    composition(lambda: call(torch.bfloat16))
    monkeypatch.setenv("LSS_CAMERA_BRANCH_TRAIN_NATIVE", "1")
    composition(lambda: call(torch.float16))

    def no_grad():
        with torch.no_grad(), torch.autocast(**BF16):
            m.scene_tokens(c3)

    composition(no_grad)
    m96 = mv.VoVNetBEVTransformer(1, GRID_COARSE, dict(final_dim=(128, 352), Ncams=6, cams=list("abcdef")), outC=4,
                                  backbone=_Trunk(96, 128), precision="bf16").cuda().train()

    def foreign_width():
        with torch.autocast(**BF16):
            m96.scene_tokens(_c3(9, 2, cin=96).requires_grad_(True))

    composition(foreign_width)
