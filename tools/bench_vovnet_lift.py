"""The vovnet lift-splat level, training direction: forward + backward of `VoVNetBEVTransformer.get_voxels` on the
native nodes (`_HeadProjFn`, `_HeadsLiftSplatFn`: K2v / K5 forward, K7 / K10 backward) against the torch composition
(LSS_VOVNET_LIFT_NATIVE=0) in one process, at config-4 shapes (batch 8, 6 cameras, 768 / 1024-channel maps 8 x 22 /
4 x 11, v1 and v2).  Plus K10 alone against the matmul / bmm / sums form at the config-2 shape.

    python tools/bench_vovnet_lift.py [--batch 8] [--iters 20] [--warmup 5] [--rounds 2]

HIP-event times of forward + backward (median, min, max over --iters, the two paths alternating in --rounds blocks);
peak allocation increase (torch.cuda.max_memory_allocated delta) of one forward + backward.  One JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lss2_multimodal_nu_amd as L  # noqa: E402
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from lss2_multimodal_nu_amd.data import prepare_calibration  # noqa: E402
from oracle import lss_oracle as lo  # noqa: E402

GRID = dict(xbound=[-50.0, 50.0, 0.5], ybound=[-50.0, 50.0, 0.5], zbound=[-10.0, 10.0, 20.0],
            dbound=[4.0, 45.0, 1.0])


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def step(m, c3, c4, calib, G):
    bev = m.get_voxels(c3, c4, *calib)
    (bev * G).sum().backward()


def timed(m, c3, c4, calib, G, native, iters, warmup):
    os.environ["LSS_VOVNET_LIFT_NATIVE"] = "1" if native else "0"
    before = dict(mv.LIFT_CALLS)
    ts = []
    for i in range(warmup + iters):
        m.zero_grad(set_to_none=True)
        c3.grad = c4.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(m, c3, c4, calib, G)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    took = "native" if native else "composition"
    assert mv.LIFT_CALLS[took] == before[took] + warmup + iters, "the level did not take the %s path" % took
    return ts


def peak(m, c3, c4, calib, G, native):
    os.environ["LSS_VOVNET_LIFT_NATIVE"] = "1" if native else "0"
    m.zero_grad(set_to_none=True)
    c3.grad = c4.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(m, c3, c4, calib, G)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def level(ver, B, iters, warmup, rounds):
    conf = dict(final_dim=(128, 352), Ncams=6, cams=list("abcdef"))
    torch.manual_seed(1)
    m = L.compile_model_vovnet_transformer(B, GRID, conf, 4, lss_version=ver, precision="fp32").cuda().train()
    gen = np.random.RandomState(5)
    c3 = torch.from_numpy(gen.randn(B * 6, 768, 8, 22).astype(np.float32)).cuda().requires_grad_(True)
    c4 = torch.from_numpy(gen.randn(B * 6, 1024, 4, 11).astype(np.float32)).cuda().requires_grad_(ver == "v2")
    calib = (prepare_calibration(*lo.synthetic_rig(B, 6, train_aug=True, seed=7)), None, None, None, None)
    G = torch.randn(B, 128, 200, 200, device="cuda")
    t = {True: [], False: []}
    for r in range(rounds):  # alternating blocks, the order swapped every round
        for native in ((True, False) if r % 2 == 0 else (False, True)):
            t[native] += timed(m, c3, c4, calib, G, native, iters, warmup if r == 0 else 2)
    pk = {n: peak(m, c3, c4, calib, G, n) for n in (True, False)}
    os.environ.pop("LSS_VOVNET_LIFT_NATIVE")
    nat, comp = stats(t[True]), stats(t[False])
    return {"version": ver, "B": B, "cams": 6, "native": nat, "composition": comp,
            "speedup_median": round(comp["median_ms"] / nat["median_ms"], 3),
            "native_median_below_composition_min": nat["median_ms"] < comp["min_ms"],
            "native_peak_mib": round(pk[True] / 2 ** 20, 1), "composition_peak_mib": round(pk[False] / 2 ** 20, 1),
            "lifted_tensor_mib": round(B * 6 * 128 * 41 * 8 * 22 * 4 / 2 ** 20, 1)}


def k10_alone(iters, warmup, rounds):
    """lss_pointwise_conv_bwd (dx, dw, db; wrapper allocations included) vs the library form of
    `_LiftSplatFn.backward` at the config-2 shape."""
    BN, K, M, HW = 24, 512, 105, 176
    g = torch.randn(BN, M, HW, device="cuda")
    x = torch.randn(BN, K, HW, device="cuda")
    w = torch.randn(M, K, device="cuda")

    def lib():
        return torch.matmul(w.t().unsqueeze(0), g), torch.bmm(g, x.transpose(1, 2)).sum(0), g.sum(2).sum(0)

    def k10():
        return ops.pointwise_conv_bwd(g, x, w)

    t = {"library": [], "k10": []}
    for r in range(rounds):
        for name, f in (("library", lib), ("k10", k10)) if r % 2 == 0 else (("k10", k10), ("library", lib)):
            for i in range(warmup + iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    t[name].append(e0.elapsed_time(e1))
    return {"shape": {"BN": BN, "K": K, "M": M, "HW": HW}, "library": stats(t["library"]), "k10": stats(t["k10"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    res = {"tool": "bench_vovnet_lift", "iters_per_path": a.iters * a.rounds,
           "levels": [level(v, a.batch, a.iters, a.warmup, a.rounds) for v in ("v1", "v2")],
           "pointwise_conv_bwd_alone": k10_alone(a.iters, a.warmup, a.rounds)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
