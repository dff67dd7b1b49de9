"""One TransformerEncoderLayer training step (forward + backward) under bf16 autocast: the native route
(transformer_modules._LinearFn / _LayerNormFn / _DeformAttnFn, LSS_TRANSFORMER_NATIVE=1) against the torch
composition (LSS_TRANSFORMER_NATIVE=0: library GEMMs and layer_norm around the same sampling node), in one process.

    python tools/bench_transformer_train.py [--batches 1,8] [--hw 200] [--rounds 3] [--seconds 1.0] [--out FILE]

The legs alternate in blocks - composition, native, composition - for --rounds rounds; every leg is warmed up first;
a block is timed with HIP events over enough steps to fill --seconds.  Per leg: median / min / max of the per-step
time over the rounds, and the peak allocation increase of one step (second measurement, workspaces cached).  The
composition runs as two legs: the larger relative difference between their medians is the SPREAD of the measurement,
and `native_within_spread` says whether the native step is no slower than the faster composition leg by more than it
(the rule that decides the default of LSS_TRANSFORMER_NATIVE).  `kernels`: the new kernels alone at the
largest batch against the library call they replace (HIP-event medians).  One JSON line.

    python tools/bench_transformer_train.py --pointwise [--out profiles/r14_transformer_pointwise_bench.json]

The same protocol for the K12 nodes (`_GeluDropoutFn`, `_AddDropoutLayerNormFn`): both routes are the native one, the
legs are LSS_TRANSFORMER_POINTWISE = 0, 1, 0 (`pointwise_off_a`, `pointwise_on`, `pointwise_off_b`), and `kernels` holds
the four streaming kernels alone against the torch ops they replace, with their algorithmic bytes, the achieved bytes/s
and a bf16 `copy_` that moves the same number of bytes in the same process (the yardstick for "HBM-bound").
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


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def make_layer(dev):
    """The reference's layer with every parameter drawn (its initial offset / attention weights are zero)."""
    layer = tm.TransformerEncoderLayer(256, 8, 1024, 0.1).train()
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if name.startswith("norm") and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
            elif "sampling_offsets" not in name:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return layer.to(dev)


def inputs(B, H, dev):
    g = torch.Generator().manual_seed(B)
    src = torch.randn(B, H * H, 256, generator=g).to(dev).requires_grad_(True)
    pos = tm.PositionEmbeddingSine(128, normalize=True).table(H, H, dev).t().reshape(1, 256, H, H).expand(B, -1, -1, -1)
    ref = tm.LightweightBEVTransformer.reference_points(H, H, dev).expand(B, -1, -1)
    gw = torch.randn(B, H * H, 256, generator=g).to(dev)
    return src, pos.contiguous(), ref, gw


def step(layer, src, pos, ref, gw):
    layer.zero_grad(set_to_none=True)
    src.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(src, pos, ref)
    out.backward(gw)


# route -> (LSS_TRANSFORMER_NATIVE, LSS_TRANSFORMER_POINTWISE or None = as the caller's environment has it, counter)
ROUTES = {False: ("0", None, "composition"), True: ("1", None, "native"),
          "off": ("1", "0", "native"), "on": ("1", "1", "pointwise")}


def set_route(route):
    native, pointwise, counter = ROUTES[route]
    os.environ["LSS_TRANSFORMER_NATIVE"] = native
    if pointwise is not None:
        os.environ["LSS_TRANSFORMER_POINTWISE"] = pointwise
    return counter


def block(layer, args, native, steps):
    """`steps` steps on one route (a key of ROUTES); HIP-event time per step in ms."""
    took = set_route(native)
    before = dict(tm.TRANSFORMER_CALLS)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step(layer, *args)
    e1.record()
    torch.cuda.synchronize()
    assert tm.TRANSFORMER_CALLS[took] == before[took] + steps, "the block did not take the %s route" % took
    if native == "off":
        assert tm.TRANSFORMER_CALLS["pointwise"] == before["pointwise"]
    return e0.elapsed_time(e1) / steps


def peak(layer, args, native):
    set_route(native)
    step(layer, *args)
    layer.zero_grad(set_to_none=True)
    args[0].grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(layer, *args)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def timed(fn, iters=10, warmup=3):
    ts = []
    for i in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return round(median(ts), 4)


def kernels_alone(T, dev):
    """ops.linear_wgrad / ops.layernorm_bwd against the library calls of the composition's backward, at T tokens."""
    out = []
    g = torch.Generator().manual_seed(1)
    for name, n, k in (("offsets_logits", 192, 256), ("value_output_proj", 256, 256), ("linear1", 1024, 256),
                       ("linear2", 256, 1024)):
        x = torch.randn(T, k, generator=g).bfloat16().to(dev)
        dy = torch.randn(T, n, generator=g).bfloat16().to(dev)
        out.append({"kernel": "linear_wgrad", "layer": name, "T": T, "N": n, "K": k,
                    "native_ms": timed(lambda: ops.linear_wgrad(x, dy)),
                    "library_ms": timed(lambda: (torch.matmul(dy.t(), x), dy.sum(0)))})
        del x, dy
    x = torch.randn(T, 256, generator=g).to(dev)
    dy = torch.randn(T, 256, generator=g).to(dev)
    gamma, beta = torch.ones(256, device=dev), torch.zeros(256, device=dev)

    def lib():
        xr, gr, br = x.detach().requires_grad_(True), gamma.detach().requires_grad_(True), beta.detach().requires_grad_(True)
        F.layer_norm(xr, (256,), gr, br, 1e-5).backward(dy)

    out.append({"kernel": "layernorm_bwd", "rows": T, "native_ms": timed(lambda: ops.layernorm_bwd(x, dy, gamma, 1e-5, torch.float32)),
                "library_fwd_bwd_ms": timed(lib), "native_fwd_ms": timed(lambda: ops.layernorm(x, gamma, beta, 1e-5, torch.float32))})
    return out


def pointwise_kernels_alone(T, dev, p=0.1):
    """The four K12 kernels at T tokens against the torch ops they replace.  bytes = the algorithmic traffic (every
    operand read or written once); copy_ms = a bf16 copy_ that reads and writes that many bytes in total."""
    g = torch.Generator().manual_seed(2)
    seed = ops.dropout_seed(dev)
    out = []

    def entry(name, elems, bytes_per_elem, native_ms, **library):
        nbytes = elems * bytes_per_elem
        a = torch.empty(nbytes // 4, dtype=torch.bfloat16, device=dev)
        b = torch.empty_like(a)
        copy_ms = timed(lambda: b.copy_(a))
        e = {"kernel": name, "tokens": T, "elements": elems, "bytes_per_element": bytes_per_elem, "native_ms": native_ms,
             "native_gbs": round(nbytes / native_ms * 1e-6, 1), "copy_ms": copy_ms,
             "copy_gbs": round(nbytes / copy_ms * 1e-6, 1)}
        e.update(library)
        out.append(e)

    h = torch.randn(T, 1024, generator=g).bfloat16().to(dev)
    dy = torch.randn(T, 1024, generator=g).bfloat16().to(dev)

    def lib_fwd():
        return F.dropout(F.gelu(h), p, True)

    def lib_fwd_bwd():
        hr = h.detach().requires_grad_(True)
        F.dropout(F.gelu(hr), p, True).backward(dy)

    entry("gelu_dropout_fwd", h.numel(), 4, timed(lambda: ops.gelu_dropout(h, p, seed)), library_fwd_ms=timed(lib_fwd))
    entry("gelu_dropout_bwd", h.numel(), 6, timed(lambda: ops.gelu_dropout_bwd(h, dy, p, seed)),
          library_fwd_bwd_ms=timed(lib_fwd_bwd))
    del h, dy
    res = torch.randn(T, 256, generator=g).to(dev)
    a = torch.randn(T, 256, generator=g).bfloat16().to(dev)
    dy = torch.randn(T, 256, generator=g).to(dev)
    gamma, beta = torch.ones(256, device=dev), torch.zeros(256, device=dev)

    def ln_fwd():
        return F.layer_norm(res + F.dropout(a, p, True), (256,), gamma, beta, 1e-5)

    def ln_fwd_bwd():
        rr, ar = res.detach().requires_grad_(True), a.detach().requires_grad_(True)
        gr, br = gamma.detach().requires_grad_(True), beta.detach().requires_grad_(True)
        F.layer_norm(rr + F.dropout(ar, p, True), (256,), gr, br, 1e-5).backward(dy)

    s = ops.add_dropout_layernorm(res, a, gamma, beta, 1e-5, p, seed)[0]
    entry("add_dropout_ln_fwd", res.numel(), 14, timed(lambda: ops.add_dropout_layernorm(res, a, gamma, beta, 1e-5, p, seed)),
          library_fwd_ms=timed(ln_fwd))
    entry("add_dropout_ln_bwd", res.numel(), 14,
          timed(lambda: ops.add_dropout_layernorm_bwd(s, dy, gamma, 1e-5, torch.bfloat16, p, seed)),
          library_fwd_bwd_ms=timed(ln_fwd_bwd))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--hw", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pointwise", action="store_true", help="legs LSS_TRANSFORMER_POINTWISE = 0 / 1 / 0 on the native route")
    a = ap.parse_args()
    dev = torch.device("cuda")
    H = a.hw
    layer = make_layer(dev)
    res = {"tool": "bench_transformer_train", "H": H, "W": H, "d_model": 256, "d_ff": 1024, "dropout": 0.1,
           "autocast": "bf16", "rounds": a.rounds, "runs": []}
    legs = (("composition_a", False), ("native", True), ("composition_b", False))
    if a.pointwise:
        legs = (("pointwise_off_a", "off"), ("pointwise_on", "on"), ("pointwise_off_b", "off"))
        res["legs"] = "LSS_TRANSFORMER_POINTWISE 0 / 1 / 0, LSS_TRANSFORMER_NATIVE=1"
    base, cand = legs[0][1], legs[1][1]
    batches = [int(b) for b in a.batches.split(",")]
    for B in batches:
        args = inputs(B, H, dev)
        for native in (base, cand):                     # warm-up of both routes
            block(layer, args, native, 3)
        steps = {}
        for native in (base, cand):                     # steps per block from a two-step estimate
            steps[native] = max(2, int(a.seconds / (block(layer, args, native, 2) * 1e-3) + 0.999))
        times = {name: [] for name, _ in legs}
        for _ in range(a.rounds):
            for name, native in legs:
                times[name].append(block(layer, args, native, steps[native]))
        med = {k: median(v) for k, v in times.items()}
        ca, cb, cn = med[legs[0][0]], med[legs[2][0]], med[legs[1][0]]
        spread = abs(ca - cb) / min(ca, cb)
        bname, cname = ("pointwise_off", "pointwise_on") if a.pointwise else ("composition", "native")
        run = {"B": B, "tokens": B * H * H, "steps_per_block": {bname: steps[base], cname: steps[cand]}}
        for k, v in times.items():
            run[k + "_ms"] = {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        run[bname + "_spread"] = round(spread, 4)
        run[cname + "_over_" + bname] = round(cn / min(ca, cb), 4)
        run[cname + "_within_spread"] = bool(cn <= min(ca, cb) * (1.0 + spread))
        run[cname + "_peak_mib"] = round(peak(layer, args, cand) / 2 ** 20, 1)
        run[bname + "_peak_mib"] = round(peak(layer, args, base) / 2 ** 20, 1)
        res["runs"].append(run)
        del args
        torch.cuda.empty_cache()
    res["kernels"] = (pointwise_kernels_alone if a.pointwise else kernels_alone)(max(batches) * H * H, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
