"""K8r's shared 2 x 2 tile layout (csrc/conv_ring.hip, T22: the four strips of a workgroup form one 8 x 40 output tile
with one 10 x 42 blended patch and one 7 x 23 source window; the launcher takes it for fused-upsample shapes whose
output is a multiple of 8 x 40).  Against torch's CPU conv and the tile kernel at the tolerances of
tests/test_conv_ring_gpu.py, at batch 1, a single chunk, head_n 1 - 4, a 32-channel skip tensor at 200^2, x3 / x4
upsamples and two channel blocks; bit-reproducible run to run, ring timeout counter unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import bev_oracle as bo  # noqa: E402

BF16_UP_TOL = 1.2e-2  # tests/test_conv_ring_gpu.py: fused bilinear upsample


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from lss2_multimodal_nu_amd import ops as _ops
    return _ops


def _q(t):
    return t.bfloat16().float()


SHAPES = [
    # B, H, W, Cx, Cout, C2, up, head_n, relu
    (1, 100, 100, 64, 128, 0, 2, 1, True),     # batch 1, 200^2, 1-class head
    (2, 60, 100, 32, 128, 0, 2, 2, True),      # 120 x 200: a single 32-channel chunk, 2-class head
    (2, 100, 100, 64, 128, 0, 2, 3, False),    # 3-class head, no ReLU
    (1, 100, 100, 64, 128, 32, 2, 4, True),    # 200^2 with a 32-channel skip tensor, 4-class head
    (1, 100, 100, 64, 128, 32, 2, 0, True),    # the same without the head
    (3, 20, 40, 64, 128, 0, 4, 0, False),      # 80 x 160 from a x4 upsample
    (4, 40, 40, 96, 128, 0, 3, 0, True),       # 120 x 120 from a x3 upsample, three chunks
    (2, 60, 100, 64, 256, 64, 2, 0, True),     # 120 x 200, two 128-channel blocks, 64-channel skip tensor
]


@pytest.mark.parametrize("cfg", SHAPES)
def test_ring_tile_layout_vs_torch_and_tile_kernel(ops, report, cfg):
    B, H, W, Cx, Cout, C2, up, head_n, relu = cfg
    Hin, Win = H * up, W * up
    assert Hin % 8 == 0 and Win % 40 == 0, "test shape must take the 2 x 2 tile layout"
    assert ops.conv_ring_ok(B, H, W, Cx, C2, up, Cout, head_n), "test shape must be a ring-kernel case"
    gen = torch.Generator().manual_seed(7 + sum(int(c) for c in cfg))
    x = _q(torch.randn(B, Cx, H, W, generator=gen))
    x2 = _q(torch.randn(B, C2, Hin, Win, generator=gen)) if C2 else None
    w = _q(torch.randn(Cout, Cx + C2, 3, 3, generator=gen) * ((Cx + C2) * 9) ** -0.5)
    scale, shift = torch.rand(Cout, generator=gen) + 0.5, torch.randn(Cout, generator=gen) * 0.1
    xin = bo.upsample_bilinear_ac(x, up)
    if C2:
        xin = torch.cat([x2, xin], 1)
    ref = torch.nn.functional.conv2d(xin, w, None, padding=1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if relu:
        ref = ref.relu()
    xg = ops.nchw_to_nhwc(x.cuda(), 1)
    x2g = ops.nchw_to_nhwc(x2.cuda(), 1) if C2 else None
    wr = ops.pack_conv_weight_ring(w.cuda())
    tile_ok = Cx % 64 == 0 and C2 % 64 == 0  # the tile kernel's K block is 64 channels
    wt = ops.pack_conv_weight(w.cuda(), 1) if tile_ok else None
    sc, sh = scale.cuda(), shift.cuda()
    before = ops.N.lib().lss_conv2d_ring_timeouts()
    if head_n:
        hw, hb = torch.randn(head_n, Cout, generator=gen) * Cout ** -0.5, torch.randn(head_n, generator=gen)
        ref = torch.nn.functional.conv2d(ref, hw.view(head_n, Cout, 1, 1), hb)

        def run(wp):
            return ops.conv3x3_head_nchw(xg, wp, sc, sh, hw.cuda(), hb.cuda(), x2=x2g, up=up, relu=relu).cpu()
    else:
        def run(wp):
            y = ops.conv2d_nhwc(xg, wp, (3, 3), 1, 1, sc, sh, None, relu, x2g, up, None, 1)
            return ops.nhwc_to_nchw(y, 1).cpu()
    out = run(wr)
    old = run(wt) if tile_ok else None
    out2 = run(wr)
    assert ops.N.lib().lss_conv2d_ring_timeouts() == before, "a flag wait of the ring kernel hit its bound"
    assert out.shape == ref.shape
    tag = "x".join(str(int(c)) for c in cfg)
    assert report("k8r_t22_max_rel_" + tag, (out - ref).abs().max() / ref.abs().max()) <= BF16_UP_TOL
    assert report("k8r_t22_rel_l2_" + tag, (out - ref).norm() / ref.norm()) <= BF16_UP_TOL / 3
    if old is not None:
        assert report("k8r_t22_vs_tile_" + tag, (out - old).abs().max() / ref.abs().max()) <= 8e-3
    assert torch.equal(out, out2)  # no atomics, fixed summation order: bit-reproducible
