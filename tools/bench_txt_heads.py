"""The TXT half of BEV_TXT at inference - BevPost, the ASPP, the embedders, the Linears and the predictors - at batch
4 x 6 cameras, x (24, 512, 8, 22), in one process:

    python tools/bench_txt_heads.py [--rounds 5] [--iters 200] [--out profiles/r22_txt_heads_bench.json]

Legs, alternated round by round, each warmed up, each round one HIP-event pair around --iters calls (and the wall time
of the same loop, ended by a synchronise):
  (a) composition          `_txt_heads` on library ops in fp32: what `forward` runs with the switch off
      composition_autocast the same under bf16 autocast
      native               K13's tap-list conv + K15 through `_txt_heads` with LSS_TXT_HEADS_NATIVE=1 (eight launches)
  (b) each native launch alone, on preallocated operands
  (c) the whole eval `BEV_TXT.forward` with the switch on and off (off = the default, the parent commit's code path)
  (d) the peak allocation of one call per leg
Medians, minima and maxima go to --out as JSON, and one JSON line to stdout.  `native_beats_composition` is the rule
of DESIGN.md 4b: the native MEDIAN below the composition's MINIMUM, for the TXT half alone AND for the whole forward.
The route stays opt-in either way (tests/test_modules_gpu.py pins act / desc of the bf16 model to the fp32 heads).
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
from lss2_multimodal_nu_amd import model_BEV_TXT as mb  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from lss2_multimodal_nu_amd.modules import _to_nhwc  # noqa: E402
from oracle import lss_oracle as lo  # noqa: E402

GRID = dict(xbound=[-50.0, 50.0, 0.5], ybound=[-50.0, 50.0, 0.5], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
B, NCAM = 4, 6


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_txt_heads_bench.json"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    torch.manual_seed(0)
    conf = dict(final_dim=(128, 352), Ncams=NCAM)
    m = L.compile_model_bevtxt(B, GRID, conf, 4, precision="bf16").cuda().eval()
    gen = np.random.RandomState(22)
    x = torch.from_numpy(gen.randn(B * NCAM, 512, 8, 22).astype(np.float32)).cuda()
    calib = lo.synthetic_rig(B, NCAM, train_aug=True, seed=7)
    torch.set_grad_enabled(False)
    bev = m._bev(x, *calib)
    crop = bev.detach()[:, :, 60:140, 56:144]

    def half(flag, autocast=False):
        def run():
            os.environ["LSS_TXT_HEADS_NATIVE"] = flag
            if autocast:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return m._txt_heads(x, crop)
            return m._txt_heads(x, crop)
        return run

    before = dict(mb.TXT_HEADS_CALLS)
    half("1")()
    assert mb.TXT_HEADS_CALLS["native"] == before["native"] + 1, "the native route refused the benchmark shape"
    legs = {"composition": half("0"), "composition_autocast": half("0", True), "native": half("1")}
    res = {"tool": "bench_txt_heads", "device": torch.cuda.get_device_name(0), "B": B, "cams": NCAM,
           "x": list(x.shape), "bev": list(bev.shape), "bev_strides": list(bev.stride()), "rounds": a.rounds,
           "iters": a.iters, "unit": "ms", "txt_half_ms": alternate(legs, a.rounds, a.iters),
           "peak_mib": {k: peak(fn) for k, fn in legs.items()}}

    # (b) the native launches alone, on preallocated operands
    plan, dt, M = m._txt_plan, ops.DT_BF16, mb._TxtHeadsPlan.MID
    xn = _to_nhwc(x, dt)
    BN, H, W, _ = xn.shape
    mean = x.mean(dim=(2, 3))
    cat = torch.empty(BN, H, W, 4 * M, dtype=torch.bfloat16, device="cuda")
    scene = torch.empty(BN, H, W, M, dtype=torch.bfloat16, device="cuda")
    branches = []
    for i, f in enumerate(plan.aspp):
        w, sc, sh = f.get(dt)
        branches.append((w, f.conv.kernel_size[0], f.conv.dilation[0], sc, sh, i * M))
    _, gsc, gsh = plan.pool.get(dt)
    _, jsc, jsh = plan.project.get(dt)
    wg, wj, wjp = plan.pool.image("f32", None), plan.project.image("main", None), plan.project.image("pool", None)
    bias = ops.camera_pool_bias(mean, wg, gsc, gsh, wjp)
    _, psc, psh = plan.post.get(dt)
    pw = m.bevpost.post[0].weight.detach()
    post = ops.bev_post(crop, (0, 0), crop.shape[2:], pw, psc, psh)
    (fw, fb), (sw, sb), pred = plan.tensors(m)
    sets = [(f.get(dt)[0], f.get(dt)[1], f.get(dt)[2], lw.detach(), lb.detach())
            for f, lw, lb in ((plan.embed[0], fw, fb), (plan.embed[1], sw, sb))]
    pred = {k: v.detach() for k, v in pred.items()}
    res["launches_ms"] = alternate({
        "1_to_nhwc": lambda: _to_nhwc(x, dt),
        "2_mean": lambda: x.mean(dim=(2, 3)),
        "3_tapconv_aspp": lambda: ops.tapconv(xn, branches, y=cat),
        "4_camera_pool_bias": lambda: ops.camera_pool_bias(mean, wg, gsc, gsh, wjp),
        "5_tapconv_project": lambda: ops.tapconv(cat, [(wj, 1, 1, jsc, jsh, 0)], y=scene, img_bias=bias),
        "6_bev_post": lambda: ops.bev_post(crop, (0, 0), crop.shape[2:], pw, psc, psh),
        "7_8_txt_heads": lambda: ops.txt_heads(scene, post, sets[0], sets[1], pred, ops.TXT_HEADS_CAMS, NCAM),
    }, a.rounds, a.iters)

    def forward(flag):
        def run():
            os.environ["LSS_TXT_HEADS_NATIVE"] = flag
            return m(x, *calib)
        return run

    fwd = {"native_on": forward("1"), "native_off": forward("0")}
    res["forward_ms"] = alternate(fwd, a.rounds, a.forward_iters, 5)
    res["forward_peak_mib"] = {k: peak(fn) for k, fn in fwd.items()}
    t, f = res["txt_half_ms"], res["forward_ms"]
    res["native_beats_composition"] = bool(t["native"]["median"] < t["composition"]["min"]
                                           and t["native"]["median"] < t["composition_autocast"]["min"]
                                           and f["native_on"]["median"] < f["native_off"]["min"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
