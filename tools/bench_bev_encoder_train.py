"""Forward + backward of `BEVEncoderTransformer(128, 4)` under bf16 autocast: the native route (1x1 compress unit, the
two biased 3x3 units and the 64-channel head on the HIP kernels, LSS_BEV_ENCODER_NATIVE=1) against the torch
composition (LSS_BEV_ENCODER_NATIVE=0: library convolutions and BatchNorm around the same transformer), in one process.

    python tools/bench_bev_encoder_train.py [--batch 8] [--hw 200] [--rounds 5] [--seconds 1.0] [--out FILE]

The legs alternate in blocks - composition, native, composition - for --rounds rounds; every leg is warmed up first; a
block is timed with HIP events over enough steps to fill --seconds.  Per leg: median / min / max of the per-step time
over the rounds, and the peak allocation increase of one step (second measurement, workspaces cached).
`native_default` applies the rule that decides the default of LSS_BEV_ENCODER_NATIVE: native stays the
default only if its median lies below the minimum of both composition legs.  The loss is BCE over the fp32 logits,
the gradient reaches the input.  One JSON line; without --out it is also written to profiles/ under the next free
round number.
"""
import argparse
import json
import os
import re
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lss2_multimodal_nu_amd import model_vovnet_transformer as mv  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def step(model, x, target):
    model.zero_grad(set_to_none=True)
    x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        seg, _ = model(x)
        loss = F.binary_cross_entropy_with_logits(seg.float(), target)
    loss.backward()


def block(model, args, native, steps):
    """`steps` steps on one route; HIP-event time per step in ms."""
    os.environ["LSS_BEV_ENCODER_NATIVE"] = "1" if native else "0"
    took = "native" if native else "composition"
    before = dict(mv.BEV_ENCODER_CALLS)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step(model, *args)
    e1.record()
    torch.cuda.synchronize()
    assert mv.BEV_ENCODER_CALLS[took] == before[took] + steps, "the block did not take the %s route" % took
    return e0.elapsed_time(e1) / steps


def peak(model, args, native):
    os.environ["LSS_BEV_ENCODER_NATIVE"] = "1" if native else "0"
    step(model, *args)
    model.zero_grad(set_to_none=True)
    args[0].grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(model, *args)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def next_profile_path(name):
    rounds = [int(m.group(1)) for f in os.listdir(os.path.join(ROOT, "profiles")) for m in [re.match(r"r(\d+)_", f)] if m]
    return os.path.join(ROOT, "profiles", "r%02d_%s.json" % (max(rounds + [0]) + 1, name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hw", type=int, default=200)
    ap.add_argument("--cin", type=int, default=128)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = mv.BEVEncoderTransformer(a.cin, a.classes).to(dev).train()
    g = torch.Generator().manual_seed(1)
    B, H = a.batch, a.hw
    x = torch.randn(B, a.cin, H, H, generator=g).to(dev).requires_grad_(True)
    target = (torch.rand(B, a.classes, H, H, generator=g) > 0.7).float().to(dev)
    args = (x, target)
    legs = (("composition_a", False), ("native", True), ("composition_b", False))
    for native in (False, True):                     # warm-up of both routes
        block(model, args, native, 3)
    steps = {n: max(2, int(a.seconds / (block(model, args, n, 2) * 1e-3) + 0.999)) for n in (False, True)}
    times = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, native in legs:
            times[name].append(block(model, args, native, steps[native]))
    ops.assert_no_timeouts("bench_bev_encoder_train")
    res = {"tool": "bench_bev_encoder_train", "B": B, "H": H, "W": H, "C_in": a.cin, "classes": a.classes,
           "autocast": "bf16", "dropout": 0.1, "rounds": a.rounds,
           "steps_per_block": {"composition": steps[False], "native": steps[True]}}
    for k, v in times.items():
        res[k + "_ms"] = {"median": round(median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    comp_min = min(times["composition_a"] + times["composition_b"])
    res["composition_min_ms"] = round(comp_min, 4)
    res["native_over_composition_min"] = round(median(times["native"]) / comp_min, 4)
    res["native_default"] = bool(median(times["native"]) < comp_min)
    res["native_peak_mib"] = round(peak(model, args, True) / 2 ** 20, 1)
    res["composition_peak_mib"] = round(peak(model, args, False) / 2 ** 20, 1)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out or next_profile_path("bev_encoder_train_bench"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
