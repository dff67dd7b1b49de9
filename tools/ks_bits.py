#!/usr/bin/env python3
"""sha256[:16] of fixed-seed outputs of the five reducing K-split kernels (conv_ks.hip: three stride-1 instantiations, two
stride-2 ones; benched, ragged and odd shapes; with and without folded BN / residual / ReLU), one line each.  Run it on two builds
(LSS_HIP_LIB=<the other liblss_hip.so>) and diff the outputs to compare their bytes (profiles/r15_ks_tail_ab.txt).
    python tools/ks_bits.py"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lss2_multimodal_nu_amd import ops  # noqa: E402


def h(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:16]


S1 = [(4, 25, 25, 256, 256), (4, 50, 50, 128, 128), (4, 100, 100, 64, 64), (4, 27, 29, 256, 64), (2, 50, 44, 128, 128), (5, 41, 83, 64, 96)]
S2 = [(4, 100, 100, 64, 128), (4, 50, 50, 128, 256), (4, 53, 51, 128, 256), (3, 99, 97, 64, 128)]
for cfg in S1:
    B, H, W, Cin, Cout = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(B, H, W, Cin, generator=g).bfloat16().cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5).cuda()
    r = torch.randn(B, H, W, Cout, generator=g).bfloat16().cuda()
    sc, sh = (torch.rand(Cout, generator=g) + 0.5).cuda(), (torch.randn(Cout, generator=g) * 0.1).cuda()
    wk = ops.pack_conv_weight_ks(w)
    for tag, args in (("bn_res_relu", (sc, sh, r, True)), ("plain", (None, None, None, False)), ("bn_norelu", (sc, sh, None, False))):
        y = ops.conv2d_nhwc(x, wk, (3, 3), 1, 1, args[0], args[1], args[2], args[3], None, 1, None, 1)
        print("s1 %s %s %s" % (cfg, tag, h(y)))
for cfg in S2:
    B, H, W, Cin, Cout = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(B, H, W, Cin, generator=g).bfloat16().cuda()
    w1 = (torch.randn(Cout, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5).cuda()
    wd = (torch.randn(Cout, Cin, 1, 1, generator=g) * Cin ** -0.5).cuda()
    sc, sh = (torch.rand(2 * Cout, generator=g) + 0.5).cuda(), (torch.randn(2 * Cout, generator=g) * 0.1).cuda()
    wk = ops.pack_conv_weight_ks_s2_dual(w1, wd)
    for tag, a0, a1, relu in (("bn_relu", sc, sh, True), ("plain", None, None, False), ("bn_norelu", sc, sh, False)):
        y, y2 = ops.conv2d_ks_s2_dual_nhwc(x, wk, a0, a1, relu=relu)
        print("s2 %s %s %s %s" % (cfg, tag, h(y), h(y2)))
torch.cuda.synchronize()
print("timeouts", ops.timeout_counters())
