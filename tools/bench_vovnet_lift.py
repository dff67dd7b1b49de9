"""The vovnet lift-splat level, training direction: forward + backward of `VoVNetBEVTransformer.get_voxels` on the
native nodes (`_HeadProjFn`, `_HeadsLiftSplatFn`: K2v / K5 forward, K7 / K10 backward) against the torch composition
(LSS_VOVNET_LIFT_NATIVE=0) in one process, at config-4 shapes (batch 8, 6 cameras, 768 / 1024-channel maps 8 x 22 /
4 x 11, v1 and v2).  Plus K10 alone against the matmul / bmm / sums form at the config-2 shape.

    python tools/bench_vovnet_lift.py [--batch 8] [--iters 20] [--warmup 5] [--rounds 2]
    python tools/bench_vovnet_lift.py --heads [--rounds 3] [--out profiles/r17_depth_heads_train_bench.json]

HIP-event times of forward + backward (median, min, max over --iters, the two paths alternating in --rounds blocks);
peak allocation increase (torch.cuda.max_memory_allocated delta) of one forward + backward.  One JSON line.

--heads: the v2 level in train mode under bf16 autocast four ways - the 3x3 head units and the fusion tail both native
(LSS_DEPTH_HEADS_NATIVE / LSS_DEPTH_TAIL_NATIVE), each switched off alone, both off (the route before these units
existed) - in alternating blocks, the order rotated every round; times, peak allocation, and the kernel launches of the
tail alone (torch.profiler) on both routes.  A switch earns its native default when the all-native median lies below
the minimum over all rounds of the leg with that switch alone off.  The JSON line is also written to --out.
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


HEADS_LEGS = (("both_native", "1", "1"), ("heads_off", "0", "1"), ("tail_off", "1", "0"), ("both_off", "0", "0"))


def _set_switches(heads, tail):
    os.environ["LSS_DEPTH_HEADS_NATIVE"] = heads
    os.environ["LSS_DEPTH_TAIL_NATIVE"] = tail


def _autocast_step(m, c3, c4, calib, G):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        bev = m.get_voxels(c3, c4, *calib)
    (bev.float() * G).sum().backward()


def _tail_kernels(m, B):
    """Kernel launches of the tail alone, forward + backward from a contiguous gradient, per route."""
    from torch.profiler import ProfilerActivity, profile
    D = m.D
    g = torch.Generator(device="cuda").manual_seed(3)
    d3 = torch.randn(B * 6, D, 8, 22, device="cuda", generator=g).requires_grad_(True)
    d4 = torch.randn(B * 6, D, 4, 11, device="cuda", generator=g).requires_grad_(True)
    du = torch.randn(B * 6, D, 8, 22, device="cuda", generator=g)
    leaves = [d3, d4] + list(m.depth_net.fusion.parameters())
    out = {}
    for name, tail in (("native", "1"), ("composition", "0")):
        _set_switches("1", tail)

        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                u = mv._fuse_tail(m.depth_net.fusion, d3, d4)
            torch.autograd.grad(u, leaves, du.to(u.dtype))

        try:
            for _ in range(2):
                run()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                run()
                torch.cuda.synchronize()
            out[name] = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        except Exception as e:  # a profiler that cannot trace here must not cost the timings
            out[name] = None
            out[name + "_error"] = repr(e)[:200]
    return out


def heads_leg(B, iters, warmup, rounds):
    conf = dict(final_dim=(128, 352), Ncams=6, cams=list("abcdef"))
    torch.manual_seed(1)
    m = L.compile_model_vovnet_transformer(B, GRID, conf, 4, lss_version="v2", precision="fp32").cuda().train()
    gen = np.random.RandomState(5)
    c3 = torch.from_numpy(gen.randn(B * 6, 768, 8, 22).astype(np.float32)).cuda().requires_grad_(True)
    c4 = torch.from_numpy(gen.randn(B * 6, 1024, 4, 11).astype(np.float32)).cuda().requires_grad_(True)
    calib = (prepare_calibration(*lo.synthetic_rig(B, 6, train_aug=True, seed=7)), None, None, None, None)
    G = torch.randn(B, 128, 200, 200, device="cuda")
    keep = {k: os.environ.get(k) for k in ("LSS_DEPTH_HEADS_NATIVE", "LSS_DEPTH_TAIL_NATIVE")}
    t = {name: [] for name, _, _ in HEADS_LEGS}
    per_round = {name: [] for name, _, _ in HEADS_LEGS}
    try:
        for r in range(rounds):
            order = HEADS_LEGS[r % 4:] + HEADS_LEGS[:r % 4]
            for name, heads, tail in order:
                _set_switches(heads, tail)
                units, tails = dict(mv.HEAD_UNIT_CALLS), dict(mv.FUSE_TAIL_CALLS)
                ts = []
                n = (warmup if r == 0 else 2) + iters
                for i in range(n):
                    m.zero_grad(set_to_none=True)
                    c3.grad = c4.grad = None
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _autocast_step(m, c3, c4, calib, G)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= n - iters:
                        ts.append(e0.elapsed_time(e1))
                took_u = "native" if heads == "1" else "composition"
                took_t = "native" if tail == "1" else "composition"
                assert mv.HEAD_UNIT_CALLS[took_u] == units[took_u] + 2 * n, "the head units did not take " + took_u
                assert mv.FUSE_TAIL_CALLS[took_t] == tails[took_t] + n, "the tail did not take " + took_t
                t[name] += ts
                per_round[name].append(stats(ts))
        peaks = {}
        for name, heads, tail in HEADS_LEGS:
            _set_switches(heads, tail)
            m.zero_grad(set_to_none=True)
            c3.grad = c4.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _autocast_step(m, c3, c4, calib, G)
            torch.cuda.synchronize()
            peaks[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        kernels = _tail_kernels(m, B)
        ops.assert_no_timeouts("bench_vovnet_lift --heads")
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    res = {"tool": "bench_vovnet_lift --heads", "version": "v2", "B": B, "cams": 6, "autocast": "bf16", "rounds": rounds,
           "iters_per_leg": iters * rounds, "legs_ms": {k: stats(v) for k, v in t.items()}, "per_round_ms": per_round,
           "peak_mib": peaks, "tail_alone_kernels": kernels, "device": torch.cuda.get_device_name(0)}
    nat = res["legs_ms"]["both_native"]["median_ms"]
    for switch, leg in (("LSS_DEPTH_HEADS_NATIVE", "heads_off"), ("LSS_DEPTH_TAIL_NATIVE", "tail_off")):
        comp_min = res["legs_ms"][leg]["min_ms"]
        res[switch] = {"native_median_ms": nat, "composition_min_ms": comp_min,
                       "native_over_composition_min": round(nat / comp_min, 4), "native_default": nat < comp_min}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--heads", action="store_true", help="the depth heads' units and the fusion tail, four ways")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "r17_depth_heads_train_bench.json"))
    a = ap.parse_args()
    if a.heads:
        res = heads_leg(a.batch, a.iters, a.warmup, a.rounds)
        line = json.dumps(res)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        print(line, flush=True)
        return
    res = {"tool": "bench_vovnet_lift", "iters_per_path": a.iters * a.rounds,
           "levels": [level(v, a.batch, a.iters, a.warmup, a.rounds) for v in ("v1", "v2")],
           "pointwise_conv_bwd_alone": k10_alone(a.iters, a.warmup, a.rounds)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
