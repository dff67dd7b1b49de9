"""The stride-1 K-split kernels (csrc/conv_ks.hip) with their fragment reads between the MFMAs and the residual taken by
bounds-checked buffer loads: exact integer results at the smallest odd, ragged shape of each instantiation, for every
combination the residual request distinguishes - no residual tensor (an empty buffer: every lane reads zeros), a
residual with dead slots and pixels (offsets past the buffer's end) - with and without ReLU."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [
    # B, H, W, Cin, Cout: the smallest each variant's plan takes with odd sizes and a ragged last block
    (3, 23, 21, 256, 128),   # <18, 4, 5>: 483 pixels = 6 blocks of 80 + one of 3 (four dead tiles, 13 dead pixels)
    (2, 41, 43, 128, 128),   # <9, 4, 10>: 1763 pixels = 11 blocks of 160 + one of 3
    (1, 61, 83, 64, 128),    # <9, 2, 10>: 5063 pixels = 15 blocks of 320 + one of 263; kp = 1 finishes one tile fewer
]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from lss2_multimodal_nu_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cases():
    """Per shape: integer x in [-3, 3], w in [-2, 2], r in [-3, 3] and the fp32 CPU conv, computed once."""
    out = {}
    for cfg in SHAPES:
        B, H, W, Cin, Cout = cfg
        gen = torch.Generator().manual_seed(sum(cfg) + 1)
        x = torch.randint(-3, 4, (B, Cin, H, W), generator=gen).float()
        w = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=gen).float()
        r = torch.randint(-3, 4, (B, Cout, H, W), generator=gen).float()
        out[cfg] = (x, w, r, torch.nn.functional.conv2d(x, w, None, padding=1))
    return out


@pytest.mark.parametrize("res,relu", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("cfg", SHAPES)
def test_ks_conv_is_exact_with_and_without_a_residual(ops, cases, cfg, res, relu):
    """Every product and partial sum is an integer below 2^24 (|sum| <= 13 827 + 3), so the order of the sums does not
    matter and the output EQUALS torch's CPU result rounded with .bfloat16(): a fragment read that went to the wrong
    buffer or was used before it landed, a residual value where there is none, or a dead lane's load that came back
    non-zero and was stored, changes an integer.  (Residual without ReLU: tests/test_conv_ks_gpu.py.)"""
    B, H, W, Cin, Cout = cfg
    assert ops.conv_ks_ok(B, H, W, Cin, Cout), "test shape must be a case for the K-split kernel"
    x, w, r, conv = cases[cfg]
    want = conv + r if res else conv
    if relu:
        want = want.relu()
    want = want.permute(0, 2, 3, 1).contiguous().bfloat16()
    assert relu or float(want.float().min()) < 0
    xg = x.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    rg = r.permute(0, 2, 3, 1).contiguous().bfloat16().cuda() if res else None
    wk = ops.pack_conv_weight_ks(w.cuda())
    y = [ops.conv2d_nhwc(xg, wk, (3, 3), 1, 1, None, None, rg, relu, None, 1, None, 1) for _ in range(2)]
    assert y[0].dtype == torch.bfloat16 and torch.equal(y[0].cpu(), want)
    assert torch.equal(y[0], y[1])
