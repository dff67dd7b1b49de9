"""The six-token tail of the vovnet model at inference - the pooled BEV token, camera_transformer, bev_fusion,
unified_predictor - at batch 8 x 6 cameras with an 8 x 200 x 200 x 256 bf16 refined map, in one process:

    python tools/bench_camera_tail.py [--rounds 5] [--iters 200] [--out profiles/r21_camera_tail_bench.json]

Legs, alternated round by round, each warmed up, each round one HIP-event pair around --iters calls (and the wall time
of the same loop, ended by a synchronise):
  (a) composition   refined.float().mean((1, 2)) and the three modules on library ops: what `forward` ran before K14
      native        ops.bev_pool + ops.camera_tail through `VoVNetBEVTransformer.scene_outputs` (csrc/camera_tail.hip)
  (b) each of the two launches alone, and the pool's GB/s
  (c) the whole eval `forward` with LSS_CAMERA_TAIL_NATIVE on and off (off = the code path of the parent commit)
  (d) the peak allocation of one call per leg
Medians, minima and maxima go to --out as JSON, and one JSON line to stdout.  `native_is_default` is the rule of
DESIGN.md 4b: the native median below the composition's minimum, for the tail alone AND for the whole forward.
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
from lss2_multimodal_nu_amd import ops  # noqa: E402
from oracle import lss_oracle as lo  # noqa: E402

GRID = dict(xbound=[-50.0, 50.0, 0.5], ybound=[-50.0, 50.0, 0.5], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
B, NCAM, X, Y, D = 8, 6, 200, 200, 256


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 5), "min": round(xs[0], 5), "max": round(xs[-1], 5)}


def timed(fn, iters):
    """(device ms, wall ms) per call of `iters` back-to-back calls: a HIP-event pair, and the clock around the loop and
    the synchronise that ends it."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters


def alternate(legs, rounds, iters, warmup=20):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--forward-iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_camera_tail_bench.json"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.manual_seed(0)
    conf = dict(final_dim=(128, 352), Ncams=NCAM, cams=list("abcdef"))
    m = L.compile_model_vovnet_transformer(B, GRID, conf, 4, lss_version="v2", precision="bf16").cuda().eval()
    gen = np.random.RandomState(21)
    c3 = torch.from_numpy(gen.randn(B * NCAM, 768, 8, 22).astype(np.float32)).cuda()
    c4 = torch.from_numpy(gen.randn(B * NCAM, 1024, 4, 11).astype(np.float32)).cuda()
    calib = lo.synthetic_rig(B, NCAM, train_aug=True, seed=7)
    tokens = torch.from_numpy(gen.randn(B, NCAM, D).astype(np.float32)).cuda()
    refined = torch.randn(B, X, Y, D, device="cuda").bfloat16()
    torch.set_grad_enabled(False)

    def composition():
        return m._tail(tokens, refined.float().mean(dim=(1, 2)))

    os.environ["LSS_CAMERA_TAIL_NATIVE"] = "1"
    before = dict(mv.CAMERA_TAIL_CALLS)
    m.scene_outputs(tokens, refined)
    assert mv.CAMERA_TAIL_CALLS["native"] == before["native"] + 1, "K14 refused the benchmark shape"
    legs = {"composition": composition, "native": lambda: m.scene_outputs(tokens, refined)}
    res = {"tool": "bench_camera_tail", "device": torch.cuda.get_device_name(0), "B": B, "cams": NCAM,
           "refined": [B, X, Y, D], "rounds": a.rounds, "iters": a.iters, "unit": "ms",
           "tail_ms": alternate(legs, a.rounds, a.iters),
           "peak_mib": {k: peak(fn) for k, fn in legs.items()}}
    # (b) the two launches alone, on preallocated operands
    params = m._camera_tail_native_ok(tokens, refined)
    parts = ops.bev_pool(refined)
    scale = 1.0 / (X * Y)
    per = alternate({"bev_pool": lambda: ops.bev_pool(refined),
                     "camera_tail": lambda: ops.camera_tail(tokens, params, parts, scale),
                     "float_mean": lambda: refined.float().mean(dim=(1, 2))}, a.rounds, a.iters)
    mbytes = (refined.numel() * 2 + parts.numel() * 4) / 1e6
    res["launches"] = {"bev_pool": dict(per["bev_pool"], parts=parts.shape[1], mbytes=round(mbytes, 2),
                                        gbytes_per_s_at_median=round(mbytes / per["bev_pool"]["median"], 1)),
                       "camera_tail": per["camera_tail"], "library_float_mean": per["float_mean"]}

    def forward(flag):
        def run():
            os.environ["LSS_CAMERA_TAIL_NATIVE"] = flag
            return m({"c3": c3, "c4": c4}, *calib)
        return run

    fw = {"native_on": forward("1"), "native_off": forward("0")}
    res["forward_ms"] = alternate(fw, a.rounds, a.forward_iters, 5)
    res["forward_peak_mib"] = {k: peak(fn) for k, fn in fw.items()}
    t, f = res["tail_ms"], res["forward_ms"]
    res["native_is_default"] = bool(t["native"]["median"] < t["composition"]["min"]
                                    and f["native_on"]["median"] < f["native_off"]["min"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
