#!/usr/bin/env python3
"""sha256[:16] of fixed-seed outputs of the ring kernel (conv_ring.hip) at the eight shapes of
tests/test_conv_ring_slots_gpu.py (all six instantiations: one chunk, the first refill of every slot, seven chunks, a
ragged last workgroup, the shared tile with and without the head, the per-strip fused gather, the plain head) and at the
three benched layers, one line each.  Run it on two builds (LSS_HIP_LIB=<the other liblss_hip.so>) and diff the outputs
to compare their bytes (profiles/r22_ring_slots_ab.txt).
    python tools/ring_bits.py"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lss2_multimodal_nu_amd import ops  # noqa: E402


def h(t):
    t = t.contiguous()
    return hashlib.sha256(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy().tobytes()).hexdigest()[:16]


SHAPES = [  # B, H, W, Cx, Cout, C2, up, head_n
    (4, 40, 100, 32, 256, 0, 1, 0), (4, 40, 100, 64, 256, 0, 1, 0), (4, 40, 100, 224, 256, 0, 1, 0),
    (5, 36, 90, 64, 256, 0, 1, 0), (5, 20, 40, 64, 256, 0, 2, 0), (10, 20, 40, 64, 128, 0, 2, 4),
    (4, 10, 25, 64, 256, 32, 4, 0), (4, 91, 113, 64, 128, 0, 1, 3),
    (4, 25, 25, 256, 256, 64, 4, 0), (4, 100, 100, 256, 256, 0, 1, 0), (4, 100, 100, 256, 128, 0, 2, 4),
]
for cfg in SHAPES:
    B, H, W, Cx, Cout, C2, up, hn = cfg
    assert ops.conv_ring_ok(B, H, W, Cx, C2, up, Cout, hn), cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(B, H, W, Cx, generator=g).bfloat16().cuda()
    x2 = torch.randn(B, H * up, W * up, C2, generator=g).bfloat16().cuda() if C2 else None
    w = (torch.randn(Cout, Cx + C2, 3, 3, generator=g) * ((Cx + C2) * 9) ** -0.5).cuda()
    sc, sh = (torch.rand(Cout, generator=g) + 0.5).cuda(), (torch.randn(Cout, generator=g) * 0.1).cuda()
    wr = ops.pack_conv_weight_ring(w)
    if hn:
        hw, hb = (torch.randn(hn, Cout, generator=g) * Cout ** -0.5).cuda(), torch.randn(hn, generator=g).cuda()
        for tag, relu in (("head_relu", True), ("head_norelu", False)):
            print("%s %s %s" % (cfg, tag, h(ops.conv3x3_head_nchw(x, wr, sc, sh, hw, hb, x2=x2, up=up, relu=relu))))
    else:
        for tag, a0, a1, relu in (("bn_relu", sc, sh, True), ("plain", None, None, False)):
            print("%s %s %s" % (cfg, tag, h(ops.conv2d_nhwc(x, wr, (3, 3), 1, 1, a0, a1, None, relu, x2, up, None, 1))))
torch.cuda.synchronize()
print("ring timeouts", ops.N.lib().lss_conv2d_ring_timeouts())
