"""The tail of the K-split one-pass kernels (csrc/conv_ks.hip: conv_ks_kernel<18, 4, 5> / <9, 4, 10> / <9, 2, 10> and
conv_ks_s2_dual_kernel<4> / <2>): the K parts of a tile meet in the wave that finishes it - its own part from registers,
the foreign ones through LDS - and leave through one epilogue.

1. The fp32 sum is still taken in the fixed order kp = 0 .. NKW - 1, whichever wave owns the tile.  Operands in which
   only the centre tap and ONE input channel per 32-channel chunk meet a non-zero weight: each K part contributes exactly
   one product per output, and a single product through the MFMA is exact.  The four products are a rotation of
   (2^24, 1, 1, -2^24): added in sequence they give 0 / 2 / 2 / 2 for the four rotations; every other order of the four
   adds (but the swap of the first two, which is the same sum) gives another value for at least one rotation - checked
   below on the CPU.  The rotation runs over the output channels AND over the 16-pixel tiles, so every wave meets every
   rotation both as the owner of a tile and as a sender.  With two K parts the sequence continues through the epilogue:
   (part 0, part 1, shift, residual) for the stride-1 kernel, (part 0, part 1, shift) for the stride-2 one.
2. Dead tiles and dead pixels: integer operands (every order exact), last pixel blocks shorter than one 16-pixel tile - a
   partly dead tile, tiles wholly past the block's end in the wave that owns them, and a pixel half without any live
   pixel - inside an output buffer with a canary border.  The border sees a store to an UNCLAMPED address past the
   buffer's end (the next image's pixels are only there for the images before the last).  The clamped address of a dead
   lane is the block's first pixel, inside the buffer: a store to it is seen only by the comparison of the body, and
   only if it lands after the right one."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = float(2 ** 24)
V4 = (BIG, 1.0, 1.0, -BIG)     # four K parts; two K parts + shift + residual
V3 = (BIG, 1.0, -BIG)          # two K parts + shift (the stride-2 kernel has no residual)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from lss2_multimodal_nu_amd import ops as _ops
    return _ops


def _seq(vals):
    """vals[0] + vals[1] + ... as the kernel adds them: one fp32 rounding per add, left to right."""
    s = np.float32(vals[0])
    for v in vals[1:]:
        s = np.float32(s + np.float32(v))
    return float(s)


def _rot(vals, r):
    return tuple(vals[(q + r) % len(vals)] for q in range(len(vals)))


E4 = [_seq(_rot(V4, r)) for r in range(4)]   # expected value by rotation
E3 = [_seq(_rot(V3, r)) for r in range(3)]


def test_the_reference_tells_the_orders_apart():
    """Sequential sums of the rotations: (0, 2, 2, 2) and (0, 1, 1).  Every permutation of the four adds other than the
    identity and the swap of the first two terms (a + b = b + a: the same bits) changes the value of at least one
    rotation, and so does the pairwise grouping; with three terms every order that does not start with the two parts."""
    assert E4 == [0.0, 2.0, 2.0, 2.0] and E3 == [0.0, 1.0, 1.0]
    for perm in itertools.permutations(range(4)):
        if perm in ((0, 1, 2, 3), (1, 0, 2, 3)):
            continue
        assert any(_seq([_rot(V4, r)[p] for p in perm]) != E4[r] for r in range(4)), perm
    pair = [float(np.float32(np.float32(v[0] + v[1]) + np.float32(v[2] + v[3]))) for v in (_rot(V4, r) for r in range(4))]
    assert pair != E4
    for perm in ((0, 2, 1), (1, 2, 0)):
        assert any(_seq([_rot(V3, r)[p] for p in perm]) != E3[r] for r in range(3)), perm


def _tile_rotation(B, npix):
    """m(b, p) in 0 .. 3: changes from one 16-pixel tile to the next and from image to image."""
    p = torch.arange(npix)
    return (p.div(16, rounding_mode="floor").view(1, -1) + torch.arange(B).view(-1, 1)) % 4


def _four_part_operands(B, npix, Cin, Cout, shift_rot):
    """x (B, npix, Cin): per pixel ONE channel m(b, p) of every 32-channel chunk is 1.  w (Cout, Cin), centre tap: K part
    q (Cin / 128 chunks each) has weights in ONE of its chunks only (which one alternates with the output channel), on
    the channels 0 .. 3 of that chunk: V4[(q + co + channel + shift_rot) % 4].  Output (b, p, co) = the four products
    V4[(q + co + m + shift_rot) % 4], q = 0 .. 3, one per K part."""
    m = _tile_rotation(B, npix)
    x = torch.zeros(B, npix, Cin)
    cpp = Cin // 128                                   # chunks per K part
    for c in range(Cin // 32):
        x[:, :, 32 * c:32 * c + 4] = torch.nn.functional.one_hot(m, 4).float()
    w = torch.zeros(Cout, Cin)
    co = torch.arange(Cout)
    for q in range(4):
        chunk = q * cpp + (co // 4) % cpp
        for mm in range(4):
            w[co, 32 * chunk + mm] = torch.tensor(V4)[(q + co + mm + shift_rot) % 4]
    want = torch.tensor(E4)[(co.view(1, 1, -1) + m.unsqueeze(-1) + shift_rot) % 4]
    return x, w, want


S1_ORDER_SHAPES = [
    # B, H, W, Cin, Cout: the smallest grid (64 workgroups) of each variant, and the ragged shape of test_conv_ks_gpu.py
    (1, 25, 25, 256, 256),   # four K parts of two chunks
    (1, 50, 50, 128, 128),   # four K parts of one chunk
    (1, 100, 100, 64, 64),   # two K parts x two pixel halves: the sequence goes on through shift and residual
    (4, 27, 29, 256, 64),    # last block of 63 pixels, odd width
]


@pytest.mark.parametrize("cfg", S1_ORDER_SHAPES)
def test_ks_parts_are_summed_in_order(ops, cfg):
    B, H, W, Cin, Cout = cfg
    assert ops.conv_ks_ok(B, H, W, Cin, Cout), "test shape must be a case for the K-split kernel"
    w = torch.zeros(Cout, Cin, 3, 3)
    if Cin >= 128:
        x, wc, want = _four_part_operands(B, H * W, Cin, Cout, 0)
        scale = shift = res = None
    else:
        co = torch.arange(Cout)
        seq = torch.tensor([_rot(V4, r) for r in range(4)])[co % 4]       # (Cout, 4): part 0, part 1, shift, residual
        x = torch.zeros(B, H * W, Cin)
        x[:, :, 0] = 1
        x[:, :, 32] = 1
        wc = torch.zeros(Cout, Cin)
        wc[:, 0], wc[:, 32] = seq[:, 0], seq[:, 1]
        scale, shift = torch.ones(Cout), seq[:, 2].contiguous()
        res = seq[:, 3].view(1, 1, -1).expand(B, H * W, Cout).contiguous()
        # fma(p0 + p1, 1, shift) rounds once, as the add does; then the residual
        want = torch.tensor(E4)[co % 4].view(1, 1, -1).expand(B, H * W, Cout)
    w[:, :, 1, 1] = wc
    xg = x.view(B, H, W, Cin).bfloat16().cuda()
    assert torch.equal(xg.float().cpu().view_as(x), x) and torch.equal(w.bfloat16().float(), w)   # bf16 holds them all
    rg = res.view(B, H, W, Cout).bfloat16().cuda() if res is not None else None
    sg, hg = (scale.cuda(), shift.cuda()) if shift is not None else (None, None)
    y = ops.conv2d_nhwc(xg, ops.pack_conv_weight_ks(w.cuda()), (3, 3), 1, 1, sg, hg, rg, False, None, 1, None, 1)
    got = y.float().cpu().view(B, H * W, Cout)
    assert sorted(got.unique().tolist()) == [0.0, 2.0]
    assert torch.equal(got, want.float())


S2_ORDER_SHAPES = [
    # B, H, W, Cin, Cout: the smallest case of each NKW in test_conv_ks_s2_gpu.py
    (2, 49, 51, 128, 256),   # four K parts
    (1, 126, 96, 64, 192),   # two K parts x two pixel halves: the sequence goes on through the shift
]


@pytest.mark.parametrize("cfg", S2_ORDER_SHAPES)
def test_ks_s2_parts_are_summed_in_order(ops, cfg):
    B, H, W, Cin, Cout = cfg
    assert ops.conv_ks_s2_dual_ok(B, H, W, Cin, Cout), "test shape must be a case for the stride-2 K-split kernel"
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w1 = torch.zeros(Cout, Cin, 3, 3)
    if Cin == 128:
        xo, wc1, want1 = _four_part_operands(B, Ho * Wo, Cin, Cout, 0)
        _, wcd, want2 = _four_part_operands(B, Ho * Wo, Cin, Cout, 1)      # the 1x1: one rotation further
        scale = shift = None
    else:
        co = torch.arange(Cout)
        rots = torch.tensor([_rot(V3, r) for r in range(3)])
        s1, sd = rots[co % 3], rots[(co + 1) % 3]                          # (Cout, 3): part 0, part 1, shift
        xo = torch.zeros(B, Ho * Wo, Cin)
        xo[:, :, 0] = 1
        xo[:, :, 32] = 1
        wc1, wcd = torch.zeros(Cout, Cin), torch.zeros(Cout, Cin)
        wc1[:, 0], wc1[:, 32], wcd[:, 0], wcd[:, 32] = s1[:, 0], s1[:, 1], sd[:, 0], sd[:, 1]
        scale = torch.ones(2 * Cout)
        shift = torch.cat([s1[:, 2], sd[:, 2]]).contiguous()
        want1 = torch.tensor(E3)[co % 3].view(1, 1, -1).expand(B, Ho * Wo, Cout)
        want2 = torch.tensor(E3)[(co + 1) % 3].view(1, 1, -1).expand(B, Ho * Wo, Cout)
    w1[:, :, 1, 1] = wc1
    x = torch.zeros(B, H, W, Cin)
    x[:, ::2, ::2] = xo.view(B, Ho, Wo, Cin)      # the centre tap of output (oy, ox) reads input (2 oy, 2 ox)
    wk = ops.pack_conv_weight_ks_s2_dual(w1.cuda(), wcd.view(Cout, Cin, 1, 1).contiguous().cuda())
    y, y2 = ops.conv2d_ks_s2_dual_nhwc(x.bfloat16().cuda(), wk, scale.cuda() if scale is not None else None,
                                       shift.cuda() if shift is not None else None, relu=False)
    for got, want in ((y, want1), (y2, want2)):
        got = got.float().cpu().view(B, Ho * Wo, Cout)
        assert len(got.unique()) == 2
        assert torch.equal(got, want.float())


CANARY = -1234.0      # bf16-exact, far from every output
GUARD = 8192          # elements on either side of the output


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), CANARY, dtype=torch.bfloat16, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())


S1_DEAD_SHAPES = [
    # B, H, W, Cin, Cout: last block of 7 / 7 / 4 pixels - tile 0 partly live, every other tile of the block dead
    (2, 27, 21, 256, 128),   # 567 = 7 x 80 + 7: PXT 5, the owners of tiles 1 .. 4 finish dead tiles
    (2, 47, 41, 128, 128),   # 1927 = 12 x 160 + 7: PXT 10
    (8, 4, 81, 64, 128),     # 324 = 320 + 4: two pixel halves, the second one without a live pixel
]


@pytest.mark.parametrize("cfg", S1_DEAD_SHAPES)
def test_ks_dead_tiles_are_not_stored(ops, cfg):
    """Integer operands as test_ks_conv_is_exact_on_integer_operands (|sum| <= 9 x 256 x 6 + 3 < 2^24: exact in every
    order): the output equals torch's CPU conv + residual rounded to bf16, and nothing around it was written."""
    B, H, W, Cin, Cout = cfg
    assert ops.conv_ks_ok(B, H, W, Cin, Cout), "test shape must be a case for the K-split kernel"
    assert 0 < (H * W) % {256: 80, 128: 160, 64: 320}[Cin] < 16
    gen = torch.Generator().manual_seed(sum(cfg))
    x = torch.randint(-3, 4, (B, Cin, H, W), generator=gen).float()
    w = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=gen).float()
    r = torch.randint(-3, 4, (B, Cout, H, W), generator=gen).float()
    want = (torch.nn.functional.conv2d(x, w, None, padding=1) + r).permute(0, 2, 3, 1).contiguous().bfloat16()
    xg = x.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    rg = r.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    wk = ops.pack_conv_weight_ks(w.cuda())
    buf, y = _guarded((B, H, W, Cout))
    ops._conv_launch(0, "conv2d_fwd", {"x": xg, "x2": None, "w": wk.data, "scale": None, "shift": None, "residual": rg,
                                       "y": y, "stats": None},
                     B=B, H=H, W=W, Cx=Cin, C2=0, up=1, Cout=Cout, KH=3, KW=3, stride=1, pad=1, relu=ops.W_KS,
                     dt=ops.DT_BF16)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want)
    assert _guards_intact(buf)


S2_DEAD_SHAPES = [
    # B, H, W, Cin, Cout
    (2, 49, 49, 128, 256),   # 25 x 25 = 13 x 48 + 1 outputs: one live pixel in the last block, tiles 1 and 2 dead
    (2, 99, 99, 64, 128),    # 50 x 50 = 26 x 96 + 4: two pixel halves, the second one without a live pixel
]


@pytest.mark.parametrize("cfg", S2_DEAD_SHAPES)
def test_ks_s2_dead_tiles_are_not_stored(ops, cfg):
    """As above for both outputs of the stride-2 kernel (|sum| <= 9 x 128 x 6 < 2^24)."""
    B, H, W, Cin, Cout = cfg
    assert ops.conv_ks_s2_dual_ok(B, H, W, Cin, Cout), "test shape must be a case for the stride-2 K-split kernel"
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert 0 < (Ho * Wo) % {128: 48, 64: 96}[Cin] < 16
    gen = torch.Generator().manual_seed(sum(cfg))
    x = torch.randint(-3, 4, (B, Cin, H, W), generator=gen).float()
    w1 = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=gen).float()
    wd = torch.randint(-2, 3, (Cout, Cin, 1, 1), generator=gen).float()
    want1 = torch.nn.functional.conv2d(x, w1, None, stride=2, padding=1).permute(0, 2, 3, 1).contiguous().bfloat16()
    want2 = torch.nn.functional.conv2d(x, wd, None, stride=2).permute(0, 2, 3, 1).contiguous().bfloat16()
    xg = x.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    wk = ops.pack_conv_weight_ks_s2_dual(w1.cuda(), wd.cuda())
    buf1, y = _guarded((B, Ho, Wo, Cout))
    buf2, y2 = _guarded((B, Ho, Wo, Cout))
    ops._conv_launch(4, "conv2d_fwd", {"x": xg, "w": wk.data, "scale": None, "shift": None, "y": y, "y2": y2},
                     B=B, H=H, W=W, Cx=Cin, Cout=Cout, KH=3, KW=3, stride=2, pad=1, relu=0)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want1) and torch.equal(y2.cpu(), want2)
    assert _guards_intact(buf1) and _guards_intact(buf2)
