"""Deformable-attention sampling node, training direction: forward and backward of the native node
(transformer_modules._DeformAttnFn: lss_deform_attn_pts_fwd + lss_deform_attn_bwd) against the torch composition
DeformableAttention runs with LSS_DEFORM_NATIVE=0 (batched grid_sample), in one process.

    python tools/bench_deform.py [--batches 8,1] [--hw 200] [--iters 10] [--warmup 3]

HIP-event times (median over --iters) of the forward, the backward alone and the backward's kernel entry alone;
peak allocation increase (torch.cuda.max_memory_allocated delta) of one forward + backward.  One JSON line.
"""
import argparse
import json
import os
import sys

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lss2_multimodal_nu_amd import ops  # noqa: E402
from lss2_multimodal_nu_amd import transformer_modules as tm  # noqa: E402


def torch_core(value, ol, ref, H, W):
    """DeformableAttention.forward's torch composition of the sampling core (value = value_proj output)."""
    B, N, C = value.shape
    off = ol[..., :128].reshape(B, N, 8, 8, 2)
    aw = ol[..., 128:].reshape(B, N, 8, 8).softmax(-1)
    loc = (ref[:, :, None, None, :] + off / H).clamp(0, 1)
    v = value.view(B, H, W, 8, 32).permute(0, 3, 4, 1, 2).reshape(B * 8, 32, H, W)
    grid = (loc * 2.0 - 1.0).permute(0, 2, 1, 3, 4).reshape(B * 8, N, 8, 2)
    s = F.grid_sample(v, grid, mode="bilinear", align_corners=False)
    w = aw.permute(0, 2, 1, 3).reshape(B * 8, 1, N, 8)
    return (s * w).sum(-1).view(B, 8, 32, N).permute(0, 3, 1, 2).reshape(B, N, C)


def native_core(value, ol, ref, H, W):
    return tm._DeformAttnFn.apply(value, ol, ref, H, W)


def inputs(B, H, W, dev):
    """The reference's initial sampling offsets (head direction x (p + 1), up to 8 px) plus noise, random logits."""
    g = torch.Generator().manual_seed(B)
    N = H * W
    bias = tm.DeformableAttention(256, 8, 8).sampling_offsets.bias.detach()
    off = bias.view(1, 1, 128) + torch.randn(B, N, 128, generator=g) * 0.5
    ol = torch.cat([off, torch.randn(B, N, 64, generator=g)], -1)
    val = torch.randn(B, N, 256, generator=g)
    dout = torch.randn(B, N, 256, generator=g)
    ref = tm.LightweightBEVTransformer.reference_points(H, W, dev).expand(B, -1, -1)
    return val.to(dev), ol.to(dev), ref, dout.to(dev)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def run(core, val, ol, ref, dout, H, W, iters, warmup):
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    fwd, bwd = [], []
    for i in range(warmup + iters):
        v, o = val.detach().requires_grad_(True), ol.detach().requires_grad_(True)
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        out = core(v, o, ref, H, W)
        e1.record()
        out.backward(dout)
        e2.record()
        torch.cuda.synchronize()
        if i >= warmup:
            fwd.append(e0.elapsed_time(e1))
            bwd.append(e1.elapsed_time(e2))
        del out, v, o
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v, o = val.detach().requires_grad_(True), ol.detach().requires_grad_(True)
    core(v, o, ref, H, W).backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return median(fwd), median(bwd), peak


def kernel_bwd(val, ol, ref, dout, H, W, iters, warmup):
    """lss_deform_attn_bwd alone (the wrapper's workspace / output allocations included)."""
    ts = []
    for i in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.deform_attn_bwd(val, ol, ref, dout, H, W)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,1")
    ap.add_argument("--hw", type=int, default=200)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    H = W = a.hw
    res = {"tool": "bench_deform", "H": H, "W": W, "C": 256, "runs": []}
    for B in [int(b) for b in a.batches.split(",")]:
        val, ol, ref, dout = inputs(B, H, W, dev)
        nf, nb, npk = run(native_core, val, ol, ref, dout, H, W, a.iters, a.warmup)
        kb = kernel_bwd(val, ol, ref, dout, H, W, a.iters, a.warmup)
        tf, tb, tpk = run(torch_core, val, ol, ref, dout, H, W, a.iters, a.warmup)
        res["runs"].append({
            "B": B,
            "native_fwd_ms": round(nf, 4), "native_bwd_ms": round(nb, 4), "native_bwd_kernel_ms": round(kb, 4),
            "native_fwd_bwd_ms": round(nf + nb, 4), "native_peak_mib": round(npk / 2 ** 20, 1),
            "torch_fwd_ms": round(tf, 4), "torch_bwd_ms": round(tb, 4), "torch_fwd_bwd_ms": round(tf + tb, 4),
            "torch_peak_mib": round(tpk / 2 ** 20, 1),
            "speedup_fwd_bwd": round((tf + tb) / (nf + nb), 3), "peak_ratio": round(npk / tpk, 4)})
        del val, ol, ref, dout
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
