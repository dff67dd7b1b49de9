"""A training step of the vovnet camera branch - forward + backward of `scene_tokens` under bf16 autocast - at batch
8 x 6 cameras, c3 (48, 768, 8, 22), native conv-BN units against the library composition in one process:

    python tools/bench_camera_branch_train.py [--rounds 7] [--iters 30] [--out profiles/r23_camera_branch_train_bench.json]

Legs, alternated round by round, each warmed up, each round one HIP-event pair around --iters steps (and the wall time
of the same loop, ended by a synchronise):
      composition   LSS_CAMERA_BRANCH_TRAIN_NATIVE=0: nine library conv + BatchNorm pairs in both directions
      native        LSS_CAMERA_BRANCH_TRAIN_NATIVE=1: the HIP units (K13's tap-list conv, K16, the fused 3x3 and 1x1 units)
A step is: parameter gradients set to None, forward, a weighted sum of the tokens, backward.  Also recorded: the peak
allocation of one step per leg, and the device kernels one step launches, counted from a kernel trace (torch.profiler's
device activity, taken after the timings with the profiler off during them).  Medians, minima and maxima go to --out as
JSON, and one JSON line to stdout.  `native_beats_composition` is the rule of DESIGN.md 4b that decides the switch's
default: the native MEDIAN below the composition's MINIMUM.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lss2_multimodal_nu_amd as L  # noqa: E402
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402

GRID = dict(xbound=[-50.0, 50.0, 2.0], ybound=[-50.0, 50.0, 2.0], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
B, NCAM = 8, 6


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 5), "min": round(xs[0], 5), "max": round(xs[-1], 5)}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters


def alternate(legs, rounds, iters, warmup=10):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    dev, wall = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            d, w = timed(fn, iters)
            dev[k].append(d)
            wall[k].append(w)
    return {k: dict(stats(dev[k]), wall=stats(wall[k])) for k in legs}


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def kernel_count(fn):
    """Device kernels of ONE step, from a kernel trace; None when the profiler records no device activity here."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
            and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_camera_branch_train_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera_branch_train needs the GPU: a CPU run measures nothing")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.manual_seed(0)
    conf = dict(final_dim=(128, 352), Ncams=NCAM, cams=list("abcdef"))
    m = L.compile_model_vovnet_transformer(B, GRID, conf, 4, lss_version="v2", precision="bf16").cuda().train()
    params = [p for sub in (m.feature_pyramid, m.sceneunder) for p in sub.parameters()]
    gen = np.random.RandomState(23)
    c3 = torch.from_numpy(gen.randn(B * NCAM, 768, 8, 22).astype(np.float32)).cuda().requires_grad_(True)
    wt = torch.from_numpy(gen.randn(B * NCAM, 256).astype(np.float32)).cuda()

    def step(flag):
        def run():
            os.environ["LSS_CAMERA_BRANCH_TRAIN_NATIVE"] = flag
            for p in params:
                p.grad = None
            c3.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16):
                tok = m.scene_tokens(c3)
            (tok.float() * wt).sum().backward()
        return run

    legs = {"composition": step("0"), "native": step("1")}
    before = dict(mv.CAMERA_BRANCH_TRAIN_CALLS)
    legs["native"]()
    legs["composition"]()
    assert mv.CAMERA_BRANCH_TRAIN_CALLS == {"native": before["native"] + 1, "composition": before["composition"] + 1}, \
        "the native route refused the benchmark shape"
    res = {"tool": "bench_camera_branch_train", "device": torch.cuda.get_device_name(0), "B": B, "cams": NCAM,
           "c3": list(c3.shape), "autocast": "bf16", "rounds": a.rounds, "iters": a.iters, "unit": "ms",
           "step_ms": alternate(legs, a.rounds, a.iters), "peak_mib": {k: peak(fn) for k, fn in legs.items()}}
    try:
        res["kernels_per_step"] = {k: kernel_count(fn) for k, fn in legs.items()}
    except Exception as e:  # the trace is a count, not a timing: the timings stand without it
        res["kernels_per_step"] = {"error": "%s: %s" % (type(e).__name__, e)}
    t = res["step_ms"]
    res["native_beats_composition"] = bool(t["native"]["median"] < t["composition"]["min"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
