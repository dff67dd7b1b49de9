"""The vovnet lift-splat level as autograd nodes (`_HeadProjFn`, `_HeadsLiftSplatFn`: K2v / K5 forward, K7 / K10
backward) against a float64 CPU restatement, against the torch composition it replaces (LSS_VOVNET_LIFT_NATIVE=0), and
the fallbacks.

Yardstick: the heads as stock nn modules in double on the same state_dict, `feat_proj`, then index_add of
depth (x) feat over voxel ids from `oracle.lss_oracle.get_geometry_torch` (fp32; the id contract is exact), with
loss = (bev * G).sum() for a seeded G.

Bounds.  `dev(a)` below is the largest |a - ref| / (2e-5 max|ref| + 2e-4 |ref|): the project's rule for
fp32-accumulated gradient kernels against fp64 (test_kernels_gpu.py, K7) holds iff dev <= 1.
  - tensors K7 / K10 produce directly (feat_proj.weight / .bias, v1's last 1x1 weight and bias): dev <= 1;
  - everything that continues through torch's fp32 ops (3x3 conv / BatchNorm backward, v2's fusion tail), and the
    BEV grid itself: dev <= max(1, 2 x dev of the composition path on the same GPU and inputs).
Running statistics after a train-mode step: the BatchNorms behind the 3x3 convs see the same torch ops on the same
inputs in both paths and must match bit for bit (compared with the conv library held to its deterministic solvers,
`deterministic_library` below: left to itself it does not repeat its own bits on the small C4 map).  v2's fusion BatchNorm is fed by the 1x1 logits, which the native path
computes with K2v and the composition with the library conv, so its statistics agree to rounding (dev <= 1), not bits.

Measured (MI355X), dev of composition / native against the yardstick, largest over all tensors of a case:
small v1 eval 0.013 / 0.012, v1 train 0.014 / 0.015, v2 eval 0.025 / 0.023, v2 train 0.025 / 0.026, full-width v2
train 0.041 / 0.045 - both paths sit 20-80x inside the rule, the native one within +-30 % of the composition per
tensor.  Times and peak memory of both paths: tools/bench_vovnet_lift.py, profiles/r10_vovnet_lift_bench.json.

A bound of this file's own, not the issue's: conv biases in front of a train-mode BatchNorm have an exactly zero
gradient, so no relative rule applies; they are held to 2e-5 max|ref dw| of the same conv (`zero_grad_names`).  In
train mode that takes v2's `depth_c3.3.bias` / `depth_c4.3.bias` (K10 db outputs) out of the relative check; the eval
cases and test_pointwise_grad_gpu.py check db relatively.
"""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lss2_multimodal_nu_amd as L  # noqa: E402
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from oracle import lss_oracle as lo  # noqa: E402
from oracle import vovnet_oracle as vo  # noqa: E402

GRID = dict(xbound=[-50.0, 50.0, 0.5], ybound=[-50.0, 50.0, 0.5], zbound=[-10.0, 10.0, 20.0],
            dbound=[4.0, 45.0, 1.0])
GRID_COARSE = dict(GRID, xbound=[-50.0, 50.0, 2.0], ybound=[-50.0, 50.0, 2.0])


def t(a):
    return torch.from_numpy(np.asarray(a))


class _Trunk(mv.TrunkC3C4):
    def __init__(self, c3, c4):
        super().__init__()
        self.c3_channels, self.c4_channels = c3, c4


def small_model(ver, seed, c3c=64):
    """`small_model` of test_vovnet_gpu.py: C3 64 / C4 128 channels, 2 cameras, 4 x 6 maps, 50 x 50 grid."""
    conf = dict(final_dim=(64, 96), Ncams=2, cams=["A", "B"])
    m = L.compile_model_vovnet_transformer(1, GRID_COARSE, conf, 4, lss_version=ver, backbone=_Trunk(c3c, 128),
                                           precision="fp32")
    if c3c == 64:
        m.depth_net.load_state_dict(vo.seeded_state(vo.multiscale_depthnet_shapes(64, 128, 41) if ver == "v2"
                                                    else vo.standard_depthnet_shapes(64, 41), seed))
        m.cam_encode.load_state_dict(vo.seeded_state(vo.camencode_v2_shapes(64, 128), seed + 100))
    return m.cuda()


def full_model(ver, B):
    conf = dict(final_dim=(128, 352), Ncams=6, cams=list("abcdef"))
    torch.manual_seed(1)
    m = L.compile_model_vovnet_transformer(B, GRID, conf, 4, lss_version=ver, precision="fp32")
    m.depth_net.load_state_dict(vo.seeded_state(vo.multiscale_depthnet_shapes() if ver == "v2"
                                                else vo.standard_depthnet_shapes(), 21))
    m.cam_encode.load_state_dict(vo.seeded_state(vo.camencode_v2_shapes(), 22))
    return m.cuda()


def full_inputs(B, seed=5):
    gen = np.random.RandomState(seed)
    c3 = t(gen.randn(B * 6, 768, 8, 22).astype(np.float32))
    c4 = t(gen.randn(B * 6, 1024, 4, 11).astype(np.float32))
    return c3, c4, lo.synthetic_rig(B, 6, train_aug=True, seed=7)


def level_params(m):
    return [("depth_net." + k, p) for k, p in m.depth_net.named_parameters()] + \
           [("cam_encode." + k, p) for k, p in m.cam_encode.named_parameters()]


def run_level(m, c3, c4, calib, G, native):
    """One forward + backward of get_voxels on the GPU.  Returns {name: tensor on the CPU} and the BN buffers."""
    old = os.environ.get("LSS_VOVNET_LIFT_NATIVE")
    os.environ["LSS_VOVNET_LIFT_NATIVE"] = "1" if native else "0"
    try:
        before = dict(mv.LIFT_CALLS)
        for _, p in level_params(m):
            p.grad = None
        a = c3.cuda().requires_grad_(True)
        b = c4.cuda().requires_grad_(True)
        bev = m.get_voxels(a, b, *calib)
        (bev * G.cuda()).sum().backward()
        took = "native" if mv.LIFT_CALLS["native"] > before["native"] else "composition"
        assert mv.LIFT_CALLS[took] == before[took] + 1
        assert took == ("native" if native else "composition")
    finally:
        if old is None:
            os.environ.pop("LSS_VOVNET_LIFT_NATIVE")
        else:
            os.environ["LSS_VOVNET_LIFT_NATIVE"] = old
    out = {"bev": bev.detach().cpu(), "c3.grad": a.grad.cpu()}
    if b.grad is not None:
        out["c4.grad"] = b.grad.cpu()
    for k, p in level_params(m):
        out[k] = p.grad.detach().cpu().clone()
    return out


def yardstick(m, c3, c4, calib, G):
    """float64 on the CPU; independent of the kernels under test."""
    dn = copy.deepcopy(m.depth_net).cpu().double()
    ce = copy.deepcopy(m.cam_encode).cpu().double()
    for p in list(dn.parameters()) + list(ce.parameters()):
        p.grad = None
    a = c3.double().requires_grad_(True)
    b = c4.double().requires_grad_(True)
    B, N = calib[1].shape[:2]
    depth = dn(a, b)                                  # stock conv / BatchNorm / softmax modules (CPU: torch ops)
    feat = ce.feat_proj(a)
    BN, C, H, W = feat.shape
    D = depth.shape[1]
    rows = (depth.unsqueeze(1) * feat.unsqueeze(2)).view(B, N, C, D, H, W).permute(0, 1, 3, 4, 5, 2).reshape(-1, C)
    dx, bx, nx = lo.gen_dx_bx(m.grid_conf["xbound"], m.grid_conf["ybound"], m.grid_conf["zbound"])
    geom = lo.get_geometry_torch(m.frustum.detach().cpu(), *calib)
    idx, kept = lo.voxel_indices_np(geom.numpy(), dx.numpy(), bx.numpy(), nx.numpy())
    X, Y, Z = [int(v) for v in nx]
    assert Z == 1
    bidx = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1, 1), kept.shape)
    cell = torch.from_numpy(((bidx * X + idx[..., 0]) * Y + idx[..., 1])[kept])
    sel = torch.from_numpy(kept.reshape(-1))
    bev = torch.zeros(B * X * Y, C, dtype=torch.float64).index_add(0, cell, rows[sel])
    bev = bev.view(B, X, Y, C).permute(0, 3, 1, 2)
    (bev * G.double()).sum().backward()
    out = {"bev": bev.detach(), "c3.grad": a.grad}
    if b.grad is not None:
        out["c4.grad"] = b.grad
    for k, p in dn.named_parameters():
        out["depth_net." + k] = p.grad
    for k, p in ce.named_parameters():
        out["cam_encode." + k] = p.grad
    return out, dn


def dev(a, ref):
    a, ref = a.double().numpy(), ref.double().numpy()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    scale = 2e-5 * np.abs(ref).max() + 2e-4 * np.abs(ref)
    if not scale.max() > 0:
        return 0.0 if not np.abs(a).max() > 0 else float("inf")
    return float((np.abs(a - ref) / np.maximum(scale, 1e-300)).max())


def zero_grad_names(m, ver):
    """Biases whose gradient is exactly zero in exact arithmetic: a per-channel constant in front of a train-mode
    BatchNorm (through a linear map: the fusion 1x1, the bilinear upsample) is removed by its mean subtraction.  What
    any fp32 path returns there is the cancellation noise of a sum of output-gradient terms; it is bounded against the
    weight gradient of the same conv (sums of the same terms times O(1) activations): |g| <= 2e-5 max|ref dw|."""
    if not m.training:
        return {}
    if ver == "v1":
        return {"depth_net.depth_head.0.bias": "depth_net.depth_head.0.weight"}
    z = {"depth_net.%s.%d.bias" % (h, i): "depth_net.%s.%d.weight" % (h, i) for h in ("depth_c3", "depth_c4")
         for i in (0, 3)}
    z["depth_net.fusion.0.bias"] = "depth_net.fusion.0.weight"
    return z


def direct_names(ver):
    d = {"cam_encode.feat_proj.weight", "cam_encode.feat_proj.bias"}
    if ver == "v1":
        d |= {"depth_net.depth_head.3.weight", "depth_net.depth_head.3.bias"}
    return d


def check_parity(m, ver, c3, c4, calib, G, report, tag):
    ref, _ = yardstick(m, c3, c4, calib, G)
    state = copy.deepcopy(m.state_dict())
    comp = run_level(m, c3, c4, calib, G, native=False)
    stats_comp = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    m.load_state_dict(state)
    nat = run_level(m, c3, c4, calib, G, native=True)
    stats_nat = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    m.load_state_dict(state)
    bad = []
    zeros = zero_grad_names(m, ver)
    for k in sorted(ref):
        if k in zeros:
            lim = 2e-5 * float(ref[zeros[k]].abs().max())
            assert float(ref[k].abs().max()) <= 1e-6 * lim, k  # the yardstick agrees that it is zero
            zc, zn = float(comp[k].abs().max()) / lim, float(nat[k].abs().max()) / lim
            print("%s %-40s zero gradient: |g| / bound composition %.4f native %.4f" % (tag, k, zc, zn))
            if not zn <= 1.0:
                bad.append((k, zn, 1.0))
            continue
        dc, dn_ = dev(comp[k], ref[k]), dev(nat[k], ref[k])
        print("%s %-40s dev composition %.4f native %.4f" % (tag, k, dc, dn_))
        report("%s/%s/composition" % (tag, k), dc)
        report("%s/%s/native" % (tag, k), dn_)
        bound = 1.0 if k in direct_names(ver) else max(1.0, 2.0 * dc)
        if not dn_ <= bound:
            bad.append((k, dn_, bound))
    assert not bad, bad
    for k in stats_comp:  # closeness here; bit equality has a test of its own below
        assert dev(stats_nat[k].cpu(), stats_comp[k].cpu()) <= 1.0, k
    return nat


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_parity_small(golden, report, ver, train):
    g = golden("g10_vovnet_liftsplat_" + ver)
    m = small_model(ver, int(g["seed"]))
    m.train(train)
    calib = [t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    G = torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(3))
    check_parity(m, ver, t(g["c3"]), t(g["c4"]), calib, G, report, "small_%s_%s" % (ver, "train" if train else "eval"))


@contextlib.contextmanager
def deterministic_library():
    """Bit comparisons across the torch part of the level presuppose that the library repeats its own bits.  By
    default it does not: the 3x3 conv over the small model's 2 x 3 C4 map (128 -> 256 channels) returns results
    that differ by an ulp from call to call of `F.conv2d` on the same tensors (measured: 6 calls, 6 different bit
    patterns, max difference 2.4e-7).  The flag restricts the conv library to its deterministic solvers - for both
    paths alike; the kernels of this project have no such switch and need none."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = old


def test_library_conv_repeatability_measured():
    """The measurement behind `deterministic_library`: distinct bit patterns among 6 `F.conv2d` calls on the same
    tensors at the small model's C4 head shape, printed for the default mode (an observation about the library, not
    asserted: 6 of 6 when this was written) and asserted to be 1 under the flag - the premise of the bit tests."""
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(2, 128, 2, 3, generator=gen).cuda()
    w = (torch.randn(256, 128, 3, 3, generator=gen) / 34.0).cuda()
    b = torch.randn(256, generator=gen).cuda()

    def patterns():
        outs = [torch.nn.functional.conv2d(x, w, b, padding=1) for _ in range(6)]
        distinct = []
        for o in outs:
            if not any(torch.equal(o, d) for d in distinct):
                distinct.append(o)
        return len(distinct), max(float((o - outs[0]).abs().max()) for o in outs)

    n, d = patterns()
    print("library 3x3 conv, default mode: %d distinct results in 6 calls, max difference %.3g" % (n, d))
    with deterministic_library():
        n, d = patterns()
    print("library 3x3 conv, deterministic solvers: %d distinct results in 6 calls" % n)
    assert n == 1


def _case(golden, case):
    """(model in train mode, c3, c4, calib, G) of 'small_v1' / 'small_v2' / 'full_v2'."""
    if case == "full_v2":
        m = full_model("v2", 2).train()
        c3, c4, calib = full_inputs(2)
        return m, c3, c4, calib, torch.randn(2, 128, 200, 200, generator=torch.Generator().manual_seed(4))
    g = golden("g10_vovnet_liftsplat_" + case[-2:])
    m = small_model(case[-2:], int(g["seed"])).train()
    calib = [t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    return m, t(g["c3"]), t(g["c4"]), calib, torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(3))


@pytest.mark.parametrize("case", ["small_v1", "small_v2", "full_v2"])
def test_running_stats_equal_composition_bitwise(golden, case):
    """After a train-mode step the running statistics of the BatchNorms behind the 3x3 convs equal the composition's
    bit for bit: the nodes leave those BatchNorms and everything in front of them to the same torch ops (v2's fusion
    BatchNorm is excluded: see the module docstring)."""
    m, c3, c4, calib, G = _case(golden, case)
    state = copy.deepcopy(m.state_dict())
    stats = []
    with deterministic_library():
        for native in (False, False, True):
            m.load_state_dict(state)
            run_level(m, c3, c4, calib, G, native=native)
            stats.append({k: v.clone() for k, v in m.state_dict().items() if "running" in k and ".fusion." not in k})
    assert any(not torch.equal(stats[0][k], state[k]) for k in stats[0])  # the step did update them
    for k in stats[0]:
        assert torch.equal(stats[0][k], stats[1][k]), "the composition does not repeat itself: " + k
        assert torch.equal(stats[2][k], stats[1][k]), k


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("case", ["small_v1", "small_v2"])
def test_two_level_passes_bit_equal(golden, case, train):
    """Two native forward + backward passes of the whole level (torch 3x3 conv / BatchNorm parts included) give
    bit-equal `bev` and gradients, BatchNorm in eval and in train mode."""
    m, c3, c4, calib, G = _case(golden, case)
    m.train(train)
    state = copy.deepcopy(m.state_dict())
    with deterministic_library():
        r1 = run_level(m, c3, c4, calib, G, native=True)
        m.load_state_dict(state)
        r2 = run_level(m, c3, c4, calib, G, native=True)
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k


def test_parity_full_width(report):
    B = 2
    m = full_model("v2", B).train()
    c3, c4, calib = full_inputs(B)
    G = torch.randn(B, 128, 200, 200, generator=torch.Generator().manual_seed(4))
    check_parity(m, "v2", c3, c4, calib, G, report, "full_v2_train")


def test_feat_proj_share_of_c3_grad_is_direct(golden):
    """With the 3x3 branch detached (depth head frozen behind a detached copy of c3) c3.grad is K10's dx alone."""
    g = golden("g10_vovnet_liftsplat_v1")
    m = small_model("v1", int(g["seed"])).eval()
    calib = [t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    G = torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(3))
    c3 = t(g["c3"])
    a = c3.cuda().requires_grad_(True)
    with ops.region("lift_splat_level_train"):
        dcal = tuple(m._device_calib(a.device, *calib))
        nx = m._nx_ints()
        ws = m._workspace(2 * 41 * 4 * 6, nx[0] * nx[1] * nx[2], a.device)
        last, fp = m.depth_net.depth_head[3], m.cam_encode.feat_proj
        h = m.depth_net.depth_head[:3](a.detach())
        u, feat = mv._HeadProjFn.apply(h, last.weight, last.bias, a, fp.weight, fp.bias)
        bev = mv._HeadsLiftSplatFn.apply(u, feat, dcal, (m.frustum.detach(), m.dx.detach(), m.bx.detach()), ws,
                                         (1, 2, 41, 4, 6, 128), nx, ops.BEV_NCHW_F32)
    (bev * G.cuda()).sum().backward()
    # yardstick with the same detach
    dn = copy.deepcopy(m.depth_net).cpu().double()
    ce = copy.deepcopy(m.cam_encode).cpu().double()
    a64 = c3.double().requires_grad_(True)
    depth = torch.softmax(dn.depth_head(a64.detach()), 1)
    f64 = ce.feat_proj(a64)
    rows = (depth.unsqueeze(1) * f64.unsqueeze(2)).view(1, 2, 128, 41, 4, 6).permute(0, 1, 3, 4, 5, 2).reshape(-1, 128)
    dx, bx, nxx = lo.gen_dx_bx(GRID_COARSE["xbound"], GRID_COARSE["ybound"], GRID_COARSE["zbound"])
    idx, kept = lo.voxel_indices_np(lo.get_geometry_torch(m.frustum.detach().cpu(), *calib).numpy(), dx.numpy(),
                                    bx.numpy(), nxx.numpy())
    cell = torch.from_numpy((idx[..., 0] * 50 + idx[..., 1])[kept])
    bev64 = torch.zeros(2500, 128, dtype=torch.float64).index_add(0, cell, rows[torch.from_numpy(kept.reshape(-1))])
    (bev64.view(1, 50, 50, 128).permute(0, 3, 1, 2) * G.double()).sum().backward()
    assert dev(a.grad.cpu(), a64.grad) <= 1.0


def test_memory_full_width():
    """The lifted tensor and at least one of its copies / gradients can no longer exist."""
    B = 2
    m = full_model("v1", B).train()
    c3, c4, calib = full_inputs(B)
    G = torch.randn(B, 128, 200, 200, generator=torch.Generator().manual_seed(4)).cuda()
    a, b = c3.cuda().requires_grad_(True), c4.cuda()
    peak = {}
    for native in (True, False, True, False):
        os.environ["LSS_VOVNET_LIFT_NATIVE"] = "1" if native else "0"
        try:
            a.grad = None
            m.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            (m.get_voxels(a, b, *calib) * G).sum().backward()
            torch.cuda.synchronize()
            peak[native] = torch.cuda.max_memory_allocated() - base  # second round: workspaces are cached
        finally:
            os.environ.pop("LSS_VOVNET_LIFT_NATIVE")
    lifted = B * 6 * 128 * 41 * 8 * 22 * 4
    print("peak native %d composition %d lifted %d" % (peak[True], peak[False], lifted))
    assert peak[False] - peak[True] >= 2 * lifted


def _node_level(golden):
    """The nodes alone, hidden maps as leaves: everything downstream of them is this project's kernels, so bit
    equality is asked with the library in its default mode (`test_two_level_passes_bit_equal` covers the whole level
    with the library held to its deterministic solvers)."""
    g = golden("g10_vovnet_liftsplat_v2")
    m = small_model("v2", int(g["seed"])).eval()
    calib = [t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    c3 = t(g["c3"]).cuda().requires_grad_(True)
    with torch.no_grad():
        h3 = m.depth_net.depth_c3[:3](c3)
        h4 = m.depth_net.depth_c4[:3](t(g["c4"]).cuda())
    h3, h4 = h3.clone().requires_grad_(True), h4.clone().requires_grad_(True)
    nx = m._nx_ints()
    dcal = tuple(x.clone() for x in m._device_calib(c3.device, *calib))
    ws = m._workspace(2 * 41 * 4 * 6, nx[0] * nx[1] * nx[2], c3.device)
    consts = (m.frustum.detach(), m.dx.detach(), m.bx.detach())
    l3, l4, fp = m.depth_net.depth_c3[3], m.depth_net.depth_c4[3], m.cam_encode.feat_proj
    G = torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(3)).cuda()
    leaves = [h3, h4, c3, l3.weight, l3.bias, l4.weight, l4.bias, fp.weight, fp.bias]

    def step():
        d3, feat = mv._HeadProjFn.apply(h3, l3.weight, l3.bias, c3, fp.weight, fp.bias)
        d4 = mv._HeadProjFn.apply(h4, l4.weight, l4.bias, None, None, None)
        bev = mv._HeadsLiftSplatFn.apply(d3, feat, dcal, consts, ws, (1, 2, 41, 4, 6, 128), nx, ops.BEV_NCHW_F32)
        loss = (bev * G).sum() + d4.square().sum()
        return (bev,) + torch.autograd.grad(loss, leaves)

    return step, (h3, h4, c3)


def test_two_passes_bit_equal(golden):
    step, _ = _node_level(golden)
    r1 = [x.clone() for x in step()]
    torch.empty(1 << 20, device="cuda").normal_()
    r2 = step()
    for i, (x, y) in enumerate(zip(r1, r2)):
        assert torch.equal(x, y), i


def test_fallbacks_take_the_composition(golden):
    g = golden("g10_vovnet_liftsplat_v1")
    calib = [t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    G = torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(3))
    m = small_model("v1", int(g["seed"])).eval()
    nat = run_level(m, t(g["c3"]), t(g["c4"]), calib, G, native=True)
    comp = run_level(m, t(g["c3"]), t(g["c4"]), calib, G, native=False)  # asserts the counter inside
    ref, _ = yardstick(m, t(g["c3"]), t(g["c4"]), calib, G)
    for k in ref:
        bound = 1.0 if k in direct_names("v1") else max(1.0, 2.0 * dev(comp[k], ref[k]))
        assert dev(nat[k], ref[k]) <= bound, k
    # a grid that wants a gradient: composition, although the switch is on
    m.frustum.requires_grad_(True)
    before = dict(mv.LIFT_CALLS)
    a = t(g["c3"]).cuda().requires_grad_(True)
    bev = m.get_voxels(a, t(g["c4"]).cuda(), *calib)
    assert mv.LIFT_CALLS["composition"] == before["composition"] + 1 and mv.LIFT_CALLS["native"] == before["native"]
    assert dev(bev.detach().cpu(), ref["bev"]) <= max(1.0, 2.0 * dev(comp["bev"], ref["bev"]))
    m.frustum.requires_grad_(False)
    # heads that are not fp32 (no autocast): the nodes compute in fp32 only, the composition takes any float dtype
    md = small_model("v1", int(g["seed"])).eval()
    md.depth_net.double()
    md.cam_encode.double()
    before = dict(mv.LIFT_CALLS)
    a = t(g["c3"]).cuda().double().requires_grad_(True)
    bev = md.get_voxels(a, t(g["c4"]).cuda().double(), *calib)
    bev.sum().backward()
    assert mv.LIFT_CALLS["composition"] == before["composition"] + 1 and mv.LIFT_CALLS["native"] == before["native"]
    assert a.grad is not None and dev(bev.detach().cpu(), ref["bev"]) <= max(1.0, 2.0 * dev(comp["bev"], ref["bev"]))
    # a refused shape: 96-channel C3 (K % 64 != 0)
    torch.manual_seed(0)
    m96 = small_model("v1", 0, c3c=96).eval()
    before = dict(mv.LIFT_CALLS)
    a = torch.randn(2, 96, 4, 6, device="cuda", requires_grad=True)
    bev = m96.get_voxels(a, t(g["c4"]).cuda(), *calib)
    bev.sum().backward()
    assert mv.LIFT_CALLS["composition"] == before["composition"] + 1 and mv.LIFT_CALLS["native"] == before["native"]
    assert a.grad is not None and m96.cam_encode.feat_proj.weight.grad is not None


@pytest.mark.parametrize("amp_dtype", [torch.float16, torch.bfloat16])
def test_reference_loop_under_autocast(golden, amp_dtype):
    """The reference's training-loop body on the BEV branch: autocast, GradScaler (fp16), clip_grad_norm_(10), Adam.
    Three steps per path from the same state; an fp32 run of the native path is the middle: each autocast path's
    loss must lie within twice the composition's own distance to it (plus the 2e-4 rule), and a step with an inf in
    the loss gradient is skipped by the scaler.  The loop trains the level's parameters against a seeded BEV target.
    Measured (MI355X), losses of the three steps:
      fp32 middle       1.0050443 1.0042856 1.0038437
      fp16 native       1.0050436 1.0042850 1.0038433     fp16 composition  1.0050440 1.0042850 1.0038432
      bf16 native       1.0050396 1.0042861 1.0038429     bf16 composition  1.0050370 1.0042832 1.0038420
    i.e. distances to the middle of <= 7e-7 (fp16) and <= 7.3e-6 (bf16) for both paths."""
    g = golden("g10_vovnet_liftsplat_v2")
    calib = [t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")]
    c3, c4 = t(g["c3"]).cuda(), t(g["c4"]).cuda()
    target = torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(8)).cuda()

    def loop(native, amp, poison_step=None):
        os.environ["LSS_VOVNET_LIFT_NATIVE"] = "1" if native else "0"
        try:
            m = small_model("v2", int(g["seed"])).train()
            params = [p for _, p in level_params(m)]
            opt = torch.optim.Adam(params, lr=1e-3)
            scaler = torch.amp.GradScaler("cuda", enabled=amp == torch.float16, init_scale=1024.0)
            losses, skipped = [], []
            for step in range(3):
                opt.zero_grad()
                with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
                    bev = m.get_voxels(c3, c4, *calib)
                    loss = torch.nn.functional.mse_loss(bev.float(), target)
                if poison_step == step:
                    loss = loss * float("inf")
                before = [p.detach().clone() for p in params]
                scale0 = scaler.get_scale()
                scaler.scale(loss).backward()
                scaler.unscale_(opt)
                torch.nn.utils.clip_grad_norm_(params, 10.0)
                scaler.step(opt)
                scaler.update()
                skipped.append((scaler.get_scale() < scale0, all(torch.equal(x, y) for x, y in zip(before, params))))
                losses.append(float(loss))
            return losses, skipped
        finally:
            os.environ.pop("LSS_VOVNET_LIFT_NATIVE")

    mid, _ = loop(True, None)
    nat, _ = loop(True, amp_dtype)
    comp, _ = loop(False, amp_dtype)
    print("fp32", mid, "native", nat, "composition", comp)
    assert all(np.isfinite(v) for v in nat)
    for s in range(3):
        spread = abs(comp[s] - mid[s])  # the composition's own distance to the fp32 run
        assert abs(nat[s] - mid[s]) <= 2 * spread + 2e-4 * abs(mid[s]), (s, nat[s], comp[s], mid[s])
    if amp_dtype == torch.float16:
        _, skipped = loop(True, amp_dtype, poison_step=1)
        assert skipped[1] == (True, True)      # scale halved, parameters unchanged
        assert skipped[0][1] is False and skipped[2][1] is False


def test_capture_nodes_replay_equal_eager(golden):
    """Forward + backward of both nodes captured in one graph after eager warm-up, replayed three times on refreshed
    static inputs: every output equals the eager step's bit for bit on every replay (library in its default mode)."""
    step, statics = _node_level(golden)
    _capture_and_replay(step, statics)


def _capture_and_replay(step, statics):
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
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in static_out]
        want = step()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), (r, i)


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_capture_level_replays_equal_eager(golden, ver):
    """Forward + backward of the level as `get_voxels` runs it - 3x3 conv / BatchNorm / ReLU heads, v2's
    interpolate / cat / fusion tail, the calibration upload, both nodes - captured in one `torch.cuda.graph` after
    eager warm-up and replayed three times on refreshed static inputs: `bev` and every gradient equal the eager
    step's bit for bit on every replay.  The calibration is a pinned `CalibrationPack` (what a training loop's
    loader hands over): its upload is a copy node of the graph; the library runs on its deterministic solvers."""
    from lss2_multimodal_nu_amd.data import prepare_calibration
    g = golden("g10_vovnet_liftsplat_" + ver)
    m = small_model(ver, int(g["seed"])).eval()
    pack = prepare_calibration(*[t(g[k]) for k in ("rots", "trans", "intrins", "post_rots", "post_trans")], pin=True)
    c3 = t(g["c3"]).cuda().requires_grad_(True)
    c4 = t(g["c4"]).cuda().requires_grad_(True)
    G = torch.randn(1, 128, 50, 50, generator=torch.Generator().manual_seed(3)).cuda()
    leaves = [c3] + ([c4] if ver == "v2" else []) + [p for _, p in level_params(m)]

    def step():
        bev = m.get_voxels(c3, c4, pack, None, None, None, None)
        return (bev,) + torch.autograd.grad((bev * G).sum(), leaves)

    before = mv.LIFT_CALLS["native"]
    with deterministic_library():
        _capture_and_replay(step, (c3, c4))
    assert mv.LIFT_CALLS["native"] == before + 3 + 1 + 3  # warm-up, capture, the three eager steps: never the composition
