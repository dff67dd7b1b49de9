#!/usr/bin/env python3
"""The launch-bound 3x3 / stride-1 layers of BevEncode (layer1-3, batch 4) on the tile kernel (conv_mfma.hip) and on the
K-split one-pass kernel (conv_ks.hip), back to back inside ONE recorded launch list per kernel so that the host is out
of the picture (HIP-event timing of 40 launches per bracket); then the two stride-2 BasicBlock entries (layer2.0,
layer3.0) on the phase-plane dual launch and on the K-split kernel's stride-2 mode.   python tools/bench_ks.py [--rounds 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lss2_multimodal_nu_amd import ops  # noqa: E402

LAYERS = [("layer1 64->64 @100", 4, 100, 100, 64), ("layer2 128->128 @50", 4, 50, 50, 128), ("layer3 256->256 @25", 4, 25, 25, 256)]


S2_LAYERS = [("layer2.0 64->128 @100/2", 4, 100, 100, 64, 128), ("layer3.0 128->256 @50/2", 4, 50, 50, 128, 256)]


def _s2_operands(B, H, W, Cin, Cout):
    """x + the two weight sets of a stride-2 BasicBlock entry, packed for the phase-plane dual launch and for the K-split
    stride-2 mode."""
    x = torch.randn(B, H, W, Cin, device="cuda").bfloat16()
    w1 = torch.randn(Cout, Cin, 3, 3, device="cuda") * (Cin * 9) ** -0.5
    wd = torch.randn(Cout, Cin, 1, 1, device="cuda") * Cin ** -0.5
    sc, sh = torch.rand(2 * Cout, device="cuda") + 0.5, torch.randn(2 * Cout, device="cuda") * 0.1
    frame = torch.zeros(Cout, Cin, 3, 3, device="cuda")
    frame[:, :, 1, 1] = wd[:, :, 0, 0]
    wcat = torch.cat([ops.pack_conv_weight_s2d(w1, 1), ops.pack_conv_weight_s2d(frame, 1)], 1).contiguous()
    return x, wcat, ops.pack_conv_weight_ks_s2_dual(w1, wd), sc, sh


STEM = ("stem 7x7/2 64->64 @200", 4, 200, 200, 64)


def _stem_operands(B, H, W, Cout):
    x = torch.randn(B, H, W, 64, device="cuda").bfloat16()
    w = torch.randn(Cout, 64, 7, 7, device="cuda") * (64 * 49) ** -0.5
    sc, sh = torch.rand(Cout, device="cuda") + 0.5, torch.randn(Cout, device="cuda") * 0.1
    return x, ops.pack_conv_weight_s2d(w, 3), ops.pack_conv_weight_ks_stem(w), sc, sh


def _record(chain, launch, x):
    """One recorded launch list of `chain` launches: launch(y) -> the next y, starting from x."""
    rec = ops.ConvRecorder()
    ops.set_recorder(rec)
    y = x
    for _ in range(chain):
        y = launch(y)
    ops.set_recorder(None)
    return ops.ConvPlan(rec, x, y), x, y


def _time_plans(plans, rounds, chain):
    """plans: {key: (plan, x, y)}.  Three warm-up passes over all of them, then `rounds` HIP-event-timed passes in the
    same interleaved order; returns {key: sorted us per launch}."""
    res = {}
    for _ in range(3):
        for plan, x, y in plans.values():
            plan.run(x, y)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for key, (plan, x, y) in plans.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            plan.run(x, y)
            e.record()
            torch.cuda.synchronize()
            res.setdefault(key, []).append(s.elapsed_time(e) * 1e3 / chain)
    return {k: sorted(v) for k, v in res.items()}


def _stamped(launch):
    """The stamp buffer of one launch() after five warm-up ones."""
    for _ in range(5):
        launch()
    buf = torch.zeros(1024 * 8, dtype=torch.int64, device="cuda")
    os.environ["LSS_KS_STAMPS"] = "%x" % buf.data_ptr()
    torch.cuda.synchronize()
    launch()
    torch.cuda.synchronize()
    del os.environ["LSS_KS_STAMPS"]
    return buf


def stamps_stem():
    """Stem mode: no reduce phase (slot 4 = slot 3); 98 k-steps x 12 = 1 176 MFMAs per wave.  L2 -> CU bytes per
    workgroup, from the layout: patch 1 088 positions x 128 B = 136 KiB + weights 392 KiB requested by two waves each."""
    name, B, H, W, Cout = STEM
    x, _, wk, sc, sh = _stem_operands(B, H, W, Cout)
    _print_stamps(name, _stamped(lambda: ops.conv2d_ks_stem_nhwc(x, wk, sc, sh)), 1176.0)


def bench_stem(rounds, chain):
    """Per-launch time of the stem on the tile kernel (phase-plane form) and on the stem mode: `chain` launches over the
    same input inside one recorded list."""
    name, B, H, W, Cout = STEM
    x, ws2d, wk, sc, sh = _stem_operands(B, H, W, Cout)
    res = _time_plans({
        "tile": _record(chain, lambda _: ops.conv2d_s2_nhwc(x, ws2d, 7, 3, sc, sh, None, True), x),
        "ks": _record(chain, lambda _: ops.conv2d_ks_stem_nhwc(x, wk, sc, sh), x)}, rounds, chain)
    t, k = res["tile"], res["ks"]
    print("%-22s tile %5.2f us (min %6.2f)   ks %6.2f us (min %6.2f)   per launch incl. its boundary"
          % (name, t[len(t) // 2], t[0], k[len(k) // 2], k[0]))


def _print_stamps(name, buf, n_mfma):
    import numpy as np
    t = buf.view(-1, 8).cpu().numpy().astype(np.float64) * 0.01
    t = t[t[:, 0] != 0]
    t0 = t[:, 0].min()
    f = lambda v: "%5.2f/%5.2f" % (np.median(v), v.max())  # noqa: E731
    print("%-22s %4d | %s  %s  %s  %s  %s  %s  %s | %s" % (
        name, len(t), f(t[:, 0] - t0), f(t[:, 1] - t[:, 0]), f(t[:, 2] - t[:, 1]), f(t[:, 3] - t[:, 2]),
        f(t[:, 4] - t[:, 3]), f(t[:, 5] - t[:, 4]), f(t[:, 6] - t[:, 5]), f(t[:, 6] - t[:, 0])))
    clk = t[:, 7] * 100.0  # slot 7: s_memtime ticks over the main phase
    print("%-22s        main phase: %.0f s_memtime ticks (median) = %.1f per MFMA of a wave; ticks per us of s_memrealtime %.0f"
          % ("", np.median(clk), np.median(clk) / n_mfma, np.median(clk / np.maximum(t[:, 3] - t[:, 2], 1e-3))))


def stamps_s2():
    for name, B, H, W, Cin, Cout in S2_LAYERS:
        x, _, wk, sc, sh = _s2_operands(B, H, W, Cin, Cout)
        _print_stamps(name, _stamped(lambda: ops.conv2d_ks_s2_dual_nhwc(x, wk, sc, sh)), 120.0)


def bench_s2(rounds, chain):
    """Per-launch time of the stride-2 entries inside one recorded list: `chain` launches over the same input (the
    output is half the size, so no dependent chain; the launches still serialise on the stream)."""
    plans = {}
    for name, B, H, W, Cin, Cout in S2_LAYERS:
        x, wcat, wk, sc, sh = _s2_operands(B, H, W, Cin, Cout)
        # (_record calls its launch at once: the closures never see the next layer's operands)
        plans[(name, "dual")] = _record(chain, lambda _: ops.conv2d_s2_dual_nhwc(x, wcat, sc, sh, Cout)[0], x)
        plans[(name, "ks")] = _record(chain, lambda _: ops.conv2d_ks_s2_dual_nhwc(x, wk, sc, sh)[0], x)
    res = _time_plans(plans, rounds, chain)
    for name, *_ in S2_LAYERS:
        t, k = res[(name, "dual")], res[(name, "ks")]
        print("%-22s dual %5.2f us (min %6.2f)   ks %6.2f us (min %6.2f)   per launch incl. its boundary"
              % (name, t[len(t) // 2], t[0], k[len(k) // 2], k[0]))


def stamps():
    torch.manual_seed(0)
    print("%-22s %4s | %s" % ("K-split kernel (B=4)", "WGs", "start-spread  issue  landed  main  reduce  epilogue  drain | first->last us (p50 / max)"))
    for name, B, H, W, C in LAYERS:
        x = torch.randn(B, H, W, C, device="cuda").bfloat16()
        r = torch.randn(B, H, W, C, device="cuda").bfloat16()
        w = torch.randn(C, C, 3, 3, device="cuda") * (C * 9) ** -0.5
        sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
        wk = ops.pack_conv_weight_ks(w)
        _print_stamps(name, _stamped(lambda: ops.conv2d_nhwc(x, wk, (3, 3), 1, 1, sc, sh, r, True, None, 1, None, 1)), 180.0)
    stamps_s2()
    stamps_stem()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chain", type=int, default=40)
    ap.add_argument("--stamps", action="store_true", help="in-kernel phase stamps of the K-split kernel (one launch per layer)")
    a = ap.parse_args()
    if a.stamps:
        return stamps()
    torch.manual_seed(0)
    plans = {}
    for name, B, H, W, C in LAYERS:
        x = torch.randn(B, H, W, C, device="cuda").bfloat16()
        r = torch.randn(B, H, W, C, device="cuda").bfloat16()
        w = torch.randn(C, C, 3, 3, device="cuda") * (C * 9) ** -0.5
        sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
        for tag, wp in (("tile", ops.pack_conv_weight(w, 1)), ("ks", ops.pack_conv_weight_ks(w))):
            # a dependent chain, like the network: each launch reads the previous one's output
            plans[(name, tag)] = _record(
                a.chain, lambda y: ops.conv2d_nhwc(y, wp, (3, 3), 1, 1, sc, sh, r, True, None, 1, None, 1), x)
    res = _time_plans(plans, a.rounds, a.chain)
    for name, B, H, W, C in LAYERS:
        t, k = res[(name, "tile")], res[(name, "ks")]
        print("%-22s tile %6.2f us (min %6.2f)   ks %6.2f us (min %6.2f)   per launch incl. its boundary"
              % (name, t[len(t) // 2], t[0], k[len(k) // 2], k[0]))
    bench_s2(a.rounds, a.chain)
    bench_stem(a.rounds, a.chain)


if __name__ == "__main__":
    main()
