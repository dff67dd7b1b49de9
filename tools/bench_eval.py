"""The validation tail of one batch - what `get_val_info` does with the logits after every forward - in two forms, in one
process, at the shapes of bench.py's workload (batch 4, logits (4, 4, 200, 200) fp32, int64 targets, SimpleLoss
weights [1, 10, 5, 10]):

  composition  the torch ops written out as the reference's loop runs them: CrossEntropyLoss and `.item()`, argmax, the
               range mask, the boolean-mask index, n*a + b, bincount, reshape, add (three host round trips per batch);
  native       `ConfusionMatrix.update_from_logits` with class weights (csrc/metrics.hip: two launches per batch, no
               round trip), the loss total read once after the loop.

    python tools/bench_eval.py [--batches 200] [--pairs 5] [--warmup 20] [--out profiles/r11_eval_bench.json]

Per form and pair: wall time per batch (host clock around the loop, ending in a device synchronise - the host round
trips are the point, and HIP events alone would hide them) and HIP-event time per batch over the same loop.  The two
forms alternate, --pairs times.  A gain is claimed only when the native median lies below the composition's minimum.
The results of the two forms are compared before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lss2_multimodal_nu_amd as L  # noqa: E402

N_CLS = 4


def composition(batches, weight):
    ce = torch.nn.CrossEntropyLoss(weight=weight)
    mat = torch.zeros((N_CLS, N_CLS), dtype=torch.int64, device=weight.device)
    total = 0.0
    for preds, binimgs in batches:
        total += ce(preds, binimgs).item() * preds.shape[0]
        a, b = binimgs.flatten(), preds.argmax(1).flatten()
        k = (a >= 0) & (a < N_CLS)
        mat += torch.bincount(N_CLS * a[k].to(torch.int64) + b[k], minlength=N_CLS ** 2).reshape(N_CLS, N_CLS)
    return mat, total


def native(batches, weight):
    cm = L.ConfusionMatrix(N_CLS)
    for preds, binimgs in batches:
        cm.update_from_logits(binimgs, preds, weight)
    return cm.mat, cm.total_loss()


def timed(form, batches, weight):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    form(batches, weight)
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return wall * 1e6 / len(batches), e0.elapsed_time(e1) * 1e3 / len(batches)


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2),
            "all": [round(x, 2) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "r11_eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_eval.py measures on the GPU; none found")
    if args.pairs < 5:
        sys.exit("--pairs must be at least 5")
    g = torch.Generator().manual_seed(11)
    distinct = []
    for _ in range(4):   # four distinct batches, cycled
        t = torch.randint(0, N_CLS, (4, 200, 200), generator=g)
        t[torch.rand(4, 200, 200, generator=g) < 0.05] = -100
        distinct.append(((torch.randn(4, N_CLS, 200, 200, generator=g) * 3).cuda(), t.cuda()))
    batches = [distinct[i % 4] for i in range(args.batches)]
    weight = torch.tensor([1.0, 10.0, 5.0, 10.0], device="cuda")

    mat_c, tot_c = composition(batches, weight)
    mat_n, tot_n = native(batches, weight)
    if not torch.equal(mat_c, mat_n):
        sys.exit("the two forms disagree on the confusion matrix")
    loss_rel = abs(tot_n - tot_c) / abs(tot_c)
    if loss_rel > 2e-4:
        sys.exit("the two forms disagree on total_loss: %r vs %r" % (tot_n, tot_c))
    for form in (composition, native):
        form(batches[:args.warmup], weight)

    res = {"composition": {"wall": [], "event": []}, "native": {"wall": [], "event": []}}
    for _ in range(args.pairs):
        for name, form in (("composition", composition), ("native", native)):
            wall, ev = timed(form, batches, weight)
            res[name]["wall"].append(wall)
            res[name]["event"].append(ev)
    out = {"tool": "tools/bench_eval.py", "device": torch.cuda.get_device_name(0), "logits": [4, N_CLS, 200, 200],
           "dtype": "fp32", "batches_per_loop": args.batches, "pairs": args.pairs, "unit": "us per batch",
           "total_loss_rel_diff": loss_rel}
    for name in res:
        out[name] = {"wall_us": stats(res[name]["wall"]), "event_us": stats(res[name]["event"])}
    nat, comp = out["native"]["wall_us"], out["composition"]["wall_us"]
    out["gain_claimed"] = bool(nat["median"] < comp["min"])
    out["wall_ratio_composition_over_native"] = round(comp["median"] / nat["median"], 2)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
