"""The camera branch of the vovnet model at inference, c3 -> scene tokens, at batch 8 x 6 cameras (c3 768 x 8 x 22), in
one process:

    python tools/bench_camera_branch.py [--rounds 5] [--iters 200] [--out profiles/r19_camera_branch_bench.json]

Legs, alternated round by round, each warmed up, each round one HIP-event pair around --iters calls:
  (a) composition   sceneunder(feature_pyramid(c3)).mean((2, 3)) as eval at precision="bf16" ran it before K13: fp32
                    library ops
  (b) autocast      the same two lines under torch.autocast("cuda", torch.bfloat16)
  (c) native        VoVNetBEVTransformer.scene_tokens on K13 (csrc/camera_branch.hip)
Also: every launch of (c) alone with its shape-derived FLOPs and bytes, the whole eval `forward` with
LSS_CAMERA_BRANCH_NATIVE on and off, the peak allocation of one call per leg, and the native host calls per token call.
Medians, minima and maxima go to --out as JSON, and one JSON line to stdout.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lss2_multimodal_nu_amd as L  # noqa: E402
from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from oracle import lss_oracle as lo  # noqa: E402
from oracle import vovnet_oracle as vo  # noqa: E402

GRID = dict(xbound=[-50.0, 50.0, 0.5], ybound=[-50.0, 50.0, 0.5], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
B, NCAM, CIN, FH, FW, MID = 8, 6, 768, 8, 22, 256


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 5), "min": round(xs[0], 5), "max": round(xs[-1], 5)}


def timed(fn, iters):
    """ms per call of `iters` back-to-back calls between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(legs, rounds, iters, warmup=20):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            out[k].append(timed(fn, iters))
    return {k: stats(v) for k, v in out.items()}


def peak(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def native_launches(plan, c3):
    """(name, fn, flop, bytes) of the six launches of `_CameraBranchPlan.tokens`, on preallocated operands.  Bytes =
    activations read once + written once + the weight image once (what must cross HBM at least once)."""
    dt = ops.DT_BF16
    BN, HW = c3.shape[0], FH * FW
    Mpix = BN * HW
    x = ops.nchw_to_nhwc(c3, dt)
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=c3.device)  # noqa: E731
    pyr, p, cat = bf(BN, FH, FW, 2 * MID), bf(BN, FH, FW, MID), bf(BN, FH, FW, 4 * MID)
    b1 = [(f.get(dt)[0], 3, f.conv.dilation[0], f.get(dt)[1], f.get(dt)[2], i * MID) for i, f in enumerate(plan.pyr)]
    w, sc, sh = plan.fusion.get(dt)
    b2 = [(w, 1, 1, sc, sh, 0)]
    b3 = [(f.get(dt)[0], f.conv.kernel_size[0], f.conv.dilation[0], f.get(dt)[1], f.get(dt)[2], i * MID)
          for i, f in enumerate(plan.aspp)]
    _, gsc, gsh = plan.pool.get(dt)
    _, jsc, jsh = plan.project.get(dt)
    wg = plan.pool.image("f32", lambda w32: w32[:, :, 0, 0].contiguous())
    wj = plan.project.image("main", lambda w32: ops.pack_conv_weight(w32[:, :4 * MID].contiguous(), dt))
    wjp = plan.project.image("pool", lambda w32: w32[:, 4 * MID:, 0, 0].contiguous())
    ops.tapconv(x, b1, y=pyr)
    p_mean = ops.tapconv(pyr, b2, y=p, means=True)
    ops.tapconv(p, b3, y=cat)
    bias = ops.camera_pool_bias(p_mean, wg, gsc, gsh, wjp)
    live3 = sum(len(ops.live_taps(FH, FW, k, d)) for _, k, d, _, _, _ in b3)
    return [
        ("L0 nchw_f32_to_nhwc", lambda: ops.nchw_to_nhwc(c3, dt), 0, Mpix * CIN * 6),
        ("L1 pyramid 2 x 3x3", lambda: ops.tapconv(x, b1, y=pyr), 2 * Mpix * 18 * CIN * MID,
         2 * (Mpix * CIN + Mpix * 2 * MID + 18 * CIN * MID)),
        ("L2 fusion 1x1 + mean", lambda: ops.tapconv(pyr, b2, y=p, means=True), 2 * Mpix * 2 * MID * MID,
         2 * (Mpix * 2 * MID + Mpix * MID + 2 * MID * MID)),
        ("L3 aspp 4 branches", lambda: ops.tapconv(p, b3, y=cat), 2 * Mpix * live3 * MID * MID,
         2 * (Mpix * MID + Mpix * 4 * MID + live3 * MID * MID)),
        ("L3' pool bias", lambda: ops.camera_pool_bias(p_mean, wg, gsc, gsh, wjp), 2 * BN * 2 * MID * MID,
         4 * (2 * MID * MID + 3 * BN * MID)),
        ("L4 project + bias + mean", lambda: ops.tapconv(cat, [(wj, 1, 1, jsc, jsh, 0)], img_bias=bias, means=True),
         2 * Mpix * 4 * MID * MID, 2 * (Mpix * 4 * MID + 4 * MID * MID)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--forward-iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_camera_branch_bench.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    conf = dict(final_dim=(128, 352), Ncams=NCAM, cams=list("abcdef"))
    m = L.compile_model_vovnet_transformer(B, GRID, conf, 4, lss_version="v2", precision="bf16")
    for i, n in enumerate(("feature_pyramid", "sceneunder")):
        sub = getattr(m, n)
        sub.load_state_dict(vo.seeded_state([(k, tuple(v.shape)) for k, v in sub.state_dict().items()], 190 + i))
    m = m.cuda().eval()
    gen = np.random.RandomState(19)
    c3 = torch.from_numpy(gen.randn(B * NCAM, CIN, FH, FW).astype(np.float32)).cuda()
    c4 = torch.from_numpy(gen.randn(B * NCAM, 1024, FH // 2, FW // 2).astype(np.float32)).cuda()
    calib = lo.synthetic_rig(B, NCAM, train_aug=True, seed=7)
    torch.set_grad_enabled(False)

    def composition():
        return m.sceneunder(m.feature_pyramid(c3)).mean(dim=(2, 3))

    def autocast():
        with torch.autocast("cuda", torch.bfloat16):
            return m.sceneunder(m.feature_pyramid(c3)).mean(dim=(2, 3))

    os.environ["LSS_CAMERA_BRANCH_NATIVE"] = "1"
    before = dict(mv.CAMERA_BRANCH_CALLS)
    calls = []
    check = N.check
    N.check = lambda code, what: (calls.append(what), check(code, what))[1]
    m.scene_tokens(c3)                            # first call: packs the weights
    calls.clear()
    m.scene_tokens(c3)
    N.check = check
    assert mv.CAMERA_BRANCH_CALLS["native"] == before["native"] + 2, "K13 refused the benchmark shape"
    legs = {"composition_fp32": composition, "composition_autocast_bf16": autocast, "native": lambda: m.scene_tokens(c3)}
    res = {"tool": "bench_camera_branch", "device": torch.cuda.get_device_name(0), "B": B, "cams": NCAM,
           "c3": [B * NCAM, CIN, FH, FW], "rounds": a.rounds, "iters": a.iters, "unit": "ms",
           "tokens_ms": alternate(legs, a.rounds, a.iters),
           "peak_mib": {k: peak(fn) for k, fn in legs.items()},
           "native_host_calls": calls}
    launches = native_launches(m._camera_plan, c3)
    per = alternate({n: fn for n, fn, _, _ in launches}, a.rounds, a.iters)
    res["native_launches"] = [
        {"name": n, "ms": per[n], "gflop": round(fl / 1e9, 3), "mbytes": round(by / 1e6, 2),
         "tflops_at_median": round(fl / 1e9 / per[n]["median"], 2) if fl else None,
         "gbytes_per_s_at_median": round(by / 1e6 / per[n]["median"], 1)} for n, _, fl, by in launches]

    def forward(flag):
        def run():
            os.environ["LSS_CAMERA_BRANCH_NATIVE"] = flag
            return m({"c3": c3, "c4": c4}, *calib)
        return run

    res["forward_ms"] = alternate({"native_on": forward("1"), "native_off": forward("0")}, a.rounds, a.forward_iters, 5)
    t = res["tokens_ms"]
    res["native_is_default"] = bool(t["native"]["median"] < t["composition_fp32"]["min"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
