"""The pointwise training kernels of the BEV transformer on the GPU (K12, csrc/transformer_pointwise.hip):
`lss_gelu_dropout_fwd / _bwd` and `lss_add_dropout_ln_fwd / _bwd` through the C ABI against fp64 with the derived bounds
and the numpy mask of tests/transformer_pointwise_ref.py, the autograd nodes `_GeluDropoutFn` / `_AddDropoutLayerNormFn`,
and `TransformerEncoderLayer` with the nodes against fp64 compositions, its route, seeding, graph capture and saved
bytes.  Every test sets LSS_TRANSFORMER_NATIVE and LSS_TRANSFORMER_POINTWISE itself: none depends on a default."""
import copy
import ctypes
import math

import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

import transformer_gemm_ref as R  # noqa: E402
import transformer_grad_ref as G  # noqa: E402
import transformer_pointwise_ref as P  # noqa: E402
from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from lss2_multimodal_nu_amd import transformer_modules as tm  # noqa: E402
from test_transformer_grad_gpu import layer_inputs, make_layer, rel_l2  # noqa: E402

DT = {torch.float32: ops.DT_F32, torch.bfloat16: ops.DT_BF16}
FRONT, TAIL = 64, 4096          # guard elements of PAD_VALUE before and behind every output
SEEDS = ((P.KEY, P.STREAM), (0xF00DFACE12345678, 0x0000000100000002), (0x8000000000000001, 0xFFFFFFFFFFFFFFFF))


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _guarded(numel, dtype):
    return torch.full((FRONT + numel + TAIL,), G.PAD_VALUE, dtype=dtype, device="cuda")


def _take(buf, shape):
    n = math.prod(shape)
    out = buf[FRONT:FRONT + n].clone().reshape(shape)
    pad = torch.full((), G.PAD_VALUE, dtype=buf.dtype, device="cuda")
    assert bool((buf[:FRONT] == pad).all()) and bool((buf[FRONT + n:] == pad).all()), "guard words were written"
    return out.cpu()


def _mask(shape, p, seed):
    """(multiplier fp64, thr, scale, device seed | None) of a call."""
    if p == 0:
        return torch.ones(shape, dtype=torch.float64), 0, 1.0, None
    thr, _, scale = P.threshold(p)
    return P.multiplier(shape, p, *seed), thr, scale, P.seed_tensor(*seed, device="cuda")


def _checked(out, got, what):
    """`check` on everything but the elements whose reference overflows bf16: those must be +-inf of the right sign."""
    g = got.double()
    ov = out.overflow
    assert bool((g[ov] == torch.sign(out.ref[ov]) * float("inf")).all()), what
    ok = ~ov
    return P.check(g[ok], out.ref[ok], out.bound[ok], what)


# ----------------------------------------------------------------------------------------------------------------------
# GELU + dropout
# ----------------------------------------------------------------------------------------------------------------------
def run_gelu(h, dy, thr, scale, seed):
    hc, dyc = h.cuda(), dy.cuda()
    n = h.numel()
    ybuf, dbuf = _guarded(n, torch.bfloat16), _guarded(n, torch.bfloat16)
    sp = None if seed is None else _vp(seed)
    N.check(N.lib().lss_gelu_dropout_fwd(_vp(hc), n, thr, scale, sp, _vp(ybuf, FRONT), N.stream()), "lss_gelu_dropout_fwd")
    N.check(N.lib().lss_gelu_dropout_bwd(_vp(hc), _vp(dyc), n, thr, scale, sp, _vp(dbuf, FRONT), N.stream()),
            "lss_gelu_dropout_bwd")
    torch.cuda.synchronize()
    return _take(ybuf, h.shape), _take(dbuf, h.shape)


@pytest.mark.parametrize("p", P.PS)
@pytest.mark.parametrize("shape", P.GELU_SHAPES, ids=str)
def test_gelu_dropout_against_fp64(shape, p, report):
    h, dy = P.make_gelu_inputs(*shape)
    m, thr, scale, seed = _mask(shape, p, SEEDS[0])
    y, dh = run_gelu(h, dy, thr, scale, seed)
    fwd, bwd = P.ref_gelu_dropout(h, m, scale), P.ref_gelu_dropout_bwd(h, dy, m)
    e_y = _checked(fwd, y, "y")
    e_d = _checked(bwd, dh, "dh")
    report("gelu_dropout/%dx%d/p%.1f/y_l2" % (shape + (p,)), e_y[1])
    report("gelu_dropout/%dx%d/p%.1f/dh_l2" % (shape + (p,)), e_d[1])
    # +-3e38: finite derivative (1 or 0), never NaN
    big = h.double().abs() > 1e38
    assert bool(big.any()) and not bool(torch.isnan(dh.double()[big]).any()) and not bool(torch.isnan(y.double()).any())
    # the mask, exactly: dropped elements are exact zeros in both directions; kept ones that cannot round to zero are not
    keep = m != 0
    assert not bool(y.double()[~keep].any()) and not bool(dh.double()[~keep].any())
    for out, got in ((fwd, y), (bwd, dh)):
        must = keep & (out.ref.abs() > out.bound)
        assert bool((got.double()[must] != 0).all())
        assert int(must.sum()) >= 0.3 * int(keep.sum())       # the cases do show the mask
    if p:
        assert 0 < int((~keep).sum()) < m.numel()


def test_gelu_dropout_nan_reaches_its_own_element_only():
    shape = (5, 192)
    h, dy = P.make_gelu_inputs(*shape)
    m, thr, scale, seed = _mask(shape, 0.5, SEEDS[1])
    dropped, kept = int((m.view(-1) == 0).nonzero()[3]), int((m.view(-1) != 0).nonzero()[5])
    h = h.clone()
    h.view(-1)[dropped] = float("nan")
    h.view(-1)[kept] = float("nan")
    y, dh = run_gelu(h, dy, thr, scale, seed)
    want = torch.zeros(shape, dtype=torch.bool)
    want.view(-1)[[dropped, kept]] = True
    assert torch.equal(torch.isnan(y), want) and torch.equal(torch.isnan(dh), want)


# ----------------------------------------------------------------------------------------------------------------------
# add + dropout + LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def run_add_ln(res, a, dy, gamma, beta, thr, scale, seed):
    """Forward and backward through the C ABI on guarded outputs; the workspace starts as NaNs."""
    rows = res.shape[0]
    rc_, ac, dyc, gc, bc = (t.cuda() for t in (res, a, dy, gamma, beta))
    sp = None if seed is None else _vp(seed)
    n = rows * G.C
    sbuf, ybuf = _guarded(n, torch.float32), _guarded(n, torch.float32)
    N.check(N.lib().lss_add_dropout_ln_fwd(_vp(rc_), DT[res.dtype], _vp(ac), DT[a.dtype], rows, G.C, thr, scale, sp,
                                           _vp(gc), _vp(bc), G.EPS, _vp(sbuf, FRONT), _vp(ybuf, FRONT), N.stream()),
            "lss_add_dropout_ln_fwd")
    torch.cuda.synchronize()
    s, y = _take(sbuf, res.shape), _take(ybuf, res.shape)
    nbytes = N.lib().lss_add_dropout_ln_bwd_workspace_bytes(rows)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    dsbuf, dabuf = _guarded(n, torch.float32), _guarded(n, a.dtype)
    dgbuf, dbbuf = _guarded(G.C, torch.float32), _guarded(G.C, torch.float32)
    sc = s.cuda()
    N.check(N.lib().lss_add_dropout_ln_bwd(_vp(sc), _vp(dyc), DT[dy.dtype], _vp(gc), rows, G.C, G.EPS, thr, scale, sp,
                                           _vp(ws), nbytes, _vp(dsbuf, FRONT), _vp(dabuf, FRONT), DT[a.dtype],
                                           _vp(dgbuf, FRONT), _vp(dbbuf, FRONT), N.stream()), "lss_add_dropout_ln_bwd")
    torch.cuda.synchronize()
    return s, y, _take(dsbuf, res.shape), _take(dabuf, res.shape), _take(dgbuf, (G.C,)), _take(dbbuf, (G.C,))


@pytest.mark.parametrize("p", P.PS)
@pytest.mark.parametrize("c", P.LN_CASES, ids=lambda c: c.name)
def test_add_dropout_ln_against_fp64(c, p, report):
    for first in P.ln_firsts(c):
        res, a, dy, gamma, beta = P.make_ln_inputs(c, first)
        m, thr, scale, seed = _mask(res.shape, p, SEEDS[2])
        s, y, ds, da, dg, db = run_add_ln(res, a, dy, gamma, beta, thr, scale, seed)
        s_ref, s_bound = P.ref_add(res, a, m)
        P.check(s, s_ref, s_bound, "s")
        # everything downstream against fp64 on the kernel's own s
        y_ref, y_bound = R.ref_layernorm(s.double(), 0.0, gamma, beta, G.EPS, False)
        P.check(y, y_ref, y_bound, "y")
        ref = P.ref_add_dropout_ln_bwd(s, dy, gamma, G.EPS, m, scale, c.a_bf16)
        e = P.check(ds, ref.ds, ref.bound_ds, "ds")
        P.check(da, ref.da, ref.bound_da, "da")
        P.check(dg, ref.dgamma, ref.bound_dgamma, "dgamma")
        P.check(db, ref.dbeta, ref.bound_dbeta, "dbeta")
        report("add_dropout_ln/%s/p%.1f/ds_l2" % (c.name, p), e[1])
        # the mask, exactly
        keep = m != 0
        assert not bool(da.double()[~keep].any())
        assert torch.equal(s.double()[~keep], res.double()[~keep])
        must = keep & (ref.da.abs() > ref.bound_da)
        assert bool((da.double()[must] != 0).all())
        if c.rows >= 4:
            assert int(must.sum()) >= 0.3 * int(keep.sum())
        # one kernel template and one row text for both backwards: lss_layernorm_bwd on the same s gives the same bits
        dx2, dg2, db2 = ops.layernorm_bwd(s.cuda(), dy.cuda(), gamma.cuda(), G.EPS, torch.float32)
        for name, t2, t in (("ds", dx2, ds), ("dgamma", dg2, dg), ("dbeta", db2, db)):
            assert torch.equal(t2.cpu().view(torch.int32), t.view(torch.int32)), name
        if p == 0:  # no mask: da IS ds, rounded once where da is bf16
            if c.a_bf16:
                assert torch.equal(da.view(torch.int16), ds.bfloat16().view(torch.int16))
            else:
                assert torch.equal(da.view(torch.int32), ds.view(torch.int32))


def test_add_dropout_ln_nan_reaches_its_own_row_dgamma_and_dbeta_only():
    c = P.LN_CASES[[k.name for k in P.LN_CASES].index("rows257_resf32_abf16_dybf16")]
    res, a, dy, gamma, beta = P.make_ln_inputs(c, 0)
    m, thr, scale, seed = _mask(res.shape, 0.5, SEEDS[2])
    row = 100
    col = int((m[row] == 0).nonzero()[0])           # under a DROPPED element: NaN * 0 is NaN, as torch's mask multiply
    a = a.clone()
    a[row, col] = float("nan")
    s, y, ds, da, dg, db = run_add_ln(res, a, dy, gamma, beta, thr, scale, seed)
    rows = torch.zeros(c.rows, dtype=torch.bool)
    rows[row] = True
    only = torch.zeros_like(m, dtype=torch.bool)
    only[row, col] = True
    assert torch.equal(torch.isnan(s), only)
    for t in (y, ds, da):
        assert torch.equal(torch.isnan(t).any(-1), rows) and bool(torch.isnan(t[row]).all())
    assert bool(torch.isnan(dg).all())               # xhat of that row is NaN in every channel
    assert bool(torch.isfinite(db).all())            # dbeta = sum dy does not see s


# ----------------------------------------------------------------------------------------------------------------------
# the nodes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_dropout_node_against_fp64_autograd(p):
    shape = (257, 1024)
    h, dy = P.make_gelu_inputs(*shape)
    sane = h.double().abs() < 100            # fp64 autograd of gelu(3e38) m overflows nothing, but keep the leaf finite
    m, _, scale, seed = _mask(shape, p, SEEDS[1])
    hg = h.cuda().requires_grad_(True)
    y = tm._GeluDropoutFn.apply(hg, p, seed)
    assert y.dtype == torch.bfloat16
    y.backward(dy.cuda())
    assert hg.grad.dtype == torch.bfloat16
    h64 = h.double().requires_grad_(True)
    y64 = F.gelu(h64) * m
    y64.backward(dy.double())
    fwd, bwd = P.ref_gelu_dropout(h, m, scale), P.ref_gelu_dropout_bwd(h, dy, m)
    assert float((fwd.ref - y64.detach())[sane].abs().max()) <= 1e-12
    assert float((bwd.ref - h64.grad)[sane].abs().max()) <= 1e-12
    P.check(y.cpu().double()[sane], y64.detach()[sane], fwd.bound[sane], "node.y")
    P.check(hg.grad.cpu().double()[sane], h64.grad[sane], bwd.bound[sane], "node.dh")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", ["rows257_resf32_abf16_dybf16", "rows257_resbf16_abf16_dyf32"])
def test_add_dropout_ln_node_against_fp64_autograd(name, p):
    c = P.LN_CASES[[k.name for k in P.LN_CASES].index(name)]
    res, a, dy, gamma, beta = P.make_ln_inputs(c, 0)
    m, _, scale, seed = _mask(res.shape, p, SEEDS[2])
    leaves = [t.cuda().requires_grad_(True) for t in (res, a, gamma, beta)]
    y = tm._AddDropoutLayerNormFn.apply(leaves[0], leaves[1], leaves[2], leaves[3], G.EPS, p, seed)
    assert y.dtype == torch.float32
    y.backward(dy.cuda().float())
    assert [t.grad.dtype for t in leaves] == [res.dtype, a.dtype, torch.float32, torch.float32]
    # fp64 autograd from the kernel's own fp32 sum (the node's saved tensor: the same call gives the same bits)
    s = ops.add_dropout_layernorm(res.cuda(), a.cuda(), gamma.cuda(), beta.cuda(), G.EPS, p, seed)[0].cpu()
    P.check(s, *P.ref_add(res, a, m), "node.s")
    s64, g64, b64 = (t.double().requires_grad_(True) for t in (s, gamma, beta))
    y64 = F.layer_norm(s64, (G.C,), g64, b64, G.EPS)
    y64.backward(dy.double())
    P.check(y.cpu(), y64.detach(), R.ref_layernorm(s.double(), 0.0, gamma, beta, G.EPS, False)[1], "node.y")
    ref = P.ref_add_dropout_ln_bwd(s, dy.float(), gamma, G.EPS, m, scale, c.a_bf16)
    assert float((ref.ds - s64.grad).abs().max()) <= 1e-9
    bound_dres = R.bf16_out_bound(s64.grad, ref.bound_ds) if c.res_bf16 else ref.bound_ds
    P.check(leaves[0].grad.cpu(), s64.grad, bound_dres, "node.dres")
    P.check(leaves[1].grad.cpu(), s64.grad * m, ref.bound_da, "node.da")
    P.check(leaves[2].grad.cpu(), g64.grad, ref.bound_dgamma, "node.dgamma")
    P.check(leaves[3].grad.cpu(), b64.grad, ref.bound_dbeta, "node.dbeta")


# ----------------------------------------------------------------------------------------------------------------------
# the layer
# ----------------------------------------------------------------------------------------------------------------------
def run_layer(layer, inputs, monkeypatch, native, pointwise, device="cuda", forward=None):
    """One forward + backward under bf16 autocast (fp64 without autocast on the CPU); returns ({name: CPU tensor},
    counter deltas)."""
    src, pos, ref, Gw = (t.to(device) for t in inputs)
    if device == "cpu":
        src, pos, ref, Gw = src.double(), pos.double(), ref.double(), Gw.double()
    monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", native)
    monkeypatch.setenv("LSS_TRANSFORMER_POINTWISE", pointwise)
    layer.zero_grad(set_to_none=True)
    src = src.clone().requires_grad_(True)
    before = dict(tm.TRANSFORMER_CALLS)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=device == "cuda"):
        out = (forward or layer)(src, pos, ref)
    (out.to(Gw.dtype) * Gw).sum().backward()
    res = {"out": out.detach().cpu(), "src.grad": src.grad.cpu()}
    for k, p in layer.named_parameters():
        res[k] = p.grad.detach().cpu().clone()
    return res, {k: tm.TRANSFORMER_CALLS[k] - before[k] for k in before}


def _compare(mid, comp, nat, report, tag):
    """The rule of test_layer_native_against_composition_through_fp64: the distance of the route with the nodes to the fp64
    middle is at most twice that of the route without them, plus 2^-9 (half a bf16 ulp)."""
    assert set(nat) == set(comp) == set(mid) and len(nat) == 2 + 16
    bad = []
    for k in sorted(mid):
        assert nat[k].dtype == comp[k].dtype, k
        dc, dn = rel_l2(comp[k], mid[k]), rel_l2(nat[k], mid[k])
        print("%-40s without %.3e with %.3e" % (k, dc, dn))
        report("transformer_pointwise_layer/%s/%s/without" % (tag, k), dc)
        report("transformer_pointwise_layer/%s/%s/with" % (tag, k), dn)
        if not dn <= 2.0 * dc + 2.0 ** -9:
            bad.append((k, dn, dc))
    assert not bad, bad


def test_layer_with_the_nodes_against_composition_through_fp64(monkeypatch, report):
    """B = 2, 12 x 12 tokens, dropout 0: the fp64 composition on the CPU in the middle, the torch composition under bf16
    autocast as the yardstick, the native route with the K12 nodes as the candidate."""
    layer = make_layer(31)
    inputs = layer_inputs(2, 12, 32)
    mid, _ = run_layer(copy.deepcopy(layer).double(), inputs, monkeypatch, "0", "0", device="cpu")
    gl = copy.deepcopy(layer).cuda()
    comp, cc = run_layer(gl, inputs, monkeypatch, "0", "0")
    nat, cn = run_layer(gl, inputs, monkeypatch, "1", "1")
    assert cc == {"native": 0, "composition": 1, "pointwise": 0} and cn == {"native": 1, "composition": 0, "pointwise": 1}
    _compare(mid, comp, nat, report, "p0")


def _site_masks(B, n_tok, d_ff, p):
    """The three sites' multipliers in the order the layer draws their seeds: dropout1, dropout, dropout2."""
    shapes = ((B, n_tok, 256), (B, n_tok, d_ff), (B, n_tok, 256))
    return [P.multiplier(s, p, *seed) for s, seed in zip(shapes, SEEDS)]


def test_layer_with_dropout_against_fp64_composition_with_the_numpy_masks(monkeypatch, report):
    """B = 2, 12 x 12 tokens, p = 0.1, fixed seeds.  The middle is the fp64 composition that multiplies by the numpy
    masks; the yardstick is today's native route (switch 0) with F.dropout replaced by a multiply with the same masks,
    the candidate the route with the nodes, whose masks come from the kernels."""
    p, B, Hh, d_ff = 0.1, 2, 12, 1024
    layer = make_layer(33, dropout=p)
    inputs = layer_inputs(B, Hh, 34)
    masks = _site_masks(B, Hh * Hh, d_ff, p)

    def masked_dropout(dev):
        it = iter(masks)

        def f(x, p_, training=True, inplace=False):
            m = next(it)
            assert tuple(m.shape) == tuple(x.shape)
            return x * m.to(device=dev, dtype=x.dtype)
        return f

    monkeypatch.setattr(F, "dropout", masked_dropout("cpu"))
    mid, _ = run_layer(copy.deepcopy(layer).double(), inputs, monkeypatch, "0", "0", device="cpu")
    gl = copy.deepcopy(layer).cuda()
    monkeypatch.setattr(F, "dropout", masked_dropout("cuda"))
    comp, cc = run_layer(gl, inputs, monkeypatch, "1", "0")
    assert cc == {"native": 1, "composition": 0, "pointwise": 0}
    monkeypatch.setattr(F, "dropout", lambda *a, **k: pytest.fail("torch dropout on the route with the nodes"))
    seeds = iter([P.seed_tensor(*s, device="cuda") for s in SEEDS])
    monkeypatch.setattr(ops, "dropout_seed", lambda device: next(seeds))
    nat, cn = run_layer(gl, inputs, monkeypatch, "1", "1")
    assert cn == {"native": 1, "composition": 0, "pointwise": 1}
    _compare(mid, comp, nat, report, "p0.1")


def test_route(monkeypatch):
    """With F.gelu and F.dropout raising the layer still runs on the nodes; with the switch at 0 F.gelu is called."""
    layer = make_layer(35, dropout=0.1).cuda()
    inputs = layer_inputs(1, 8, 36)
    calls = {"gelu": 0}
    real_gelu = F.gelu

    def counting(*a, **k):
        calls["gelu"] += 1
        return real_gelu(*a, **k)

    monkeypatch.setattr(F, "gelu", counting)
    off, c0 = run_layer(layer, inputs, monkeypatch, "1", "0")
    assert calls["gelu"] == 1 and c0 == {"native": 1, "composition": 0, "pointwise": 0}

    def boom(*a, **k):
        raise AssertionError("library op on the route with the nodes")

    monkeypatch.setattr(F, "gelu", boom)
    monkeypatch.setattr(F, "dropout", boom)
    on, c1 = run_layer(layer, inputs, monkeypatch, "1", "1")
    assert c1 == {"native": 1, "composition": 0, "pointwise": 1}
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in on.values())
    # eval and dropout 0: the nodes run without a seed
    monkeypatch.setattr(ops, "dropout_seed", boom)
    run_layer(make_layer(37).cuda(), inputs, monkeypatch, "1", "1")
    layer.eval()
    _, c2 = run_layer(layer, inputs, monkeypatch, "1", "1")
    assert c2["pointwise"] == 1


def test_seeding(monkeypatch):
    layer = make_layer(38, dropout=0.1).cuda()
    inputs = layer_inputs(1, 8, 39)
    runs = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        runs.append(run_layer(layer, inputs, monkeypatch, "1", "1")[0])
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    assert not torch.equal(runs[0]["out"], runs[2]["out"])
    s1, s2 = ops.dropout_seed("cuda"), ops.dropout_seed("cuda")
    assert s1.dtype == torch.int64 and tuple(s1.shape) == (2,) and s1.is_cuda and not torch.equal(s1, s2)


def test_capture_draws_a_fresh_mask_per_replay(monkeypatch):
    """The node's forward and backward at (257, 1024), p = 0.1, the seed drawn inside the captured region: every replay
    uses ONE mask in both directions, another one than the replay before, at the right rate."""
    shape, p = (257, 1024), 0.1
    h, dy = P.make_gelu_inputs(*shape)
    v = h.double()
    live = ((P.gelu64(v).abs() > 1e-3) & (P.gelu_grad64(v).abs() > 1e-3) & (dy.double() != 0) & (v.abs() < 100)).cuda()
    assert int(live.sum()) > 0.4 * h.numel()
    hg, dyc = h.cuda().requires_grad_(True), dy.cuda()

    def step():
        y = tm._GeluDropoutFn.apply(hg, p, ops.dropout_seed(hg.device))
        return y, torch.autograd.grad(y, hg, dyc)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, dh = step()
    p_eff = P.threshold(p)[1]
    n = int(live.sum())
    sigma = math.sqrt(n * p_eff * (1.0 - p_eff))
    patterns = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        zy, zd = (y == 0) & live, (dh == 0) & live
        assert torch.equal(zy, zd)
        assert abs(int(zy.sum()) - n * p_eff) <= 6.0 * sigma
        patterns.append(zy.clone())
    assert not torch.equal(patterns[0], patterns[1]) and not torch.equal(patterns[1], patterns[2])


def test_saved_bytes(monkeypatch):
    """Bytes saved for backward by one layer forward at p = 0.1, by distinct storages: the nodes save three 16-byte seeds
    where torch saves three byte-per-element masks."""
    B, Hh, d_ff = 2, 12, 1024
    layer = make_layer(40, dropout=0.1).cuda()
    src, pos, ref, _ = (t.cuda() for t in layer_inputs(B, Hh, 41))
    src.requires_grad_(True)
    saved = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", "1")
        monkeypatch.setenv("LSS_TRANSFORMER_POINTWISE", switch)
        seen = {}

        def pack(t):
            if t.is_cuda:
                st = t.untyped_storage()
                seen[st.data_ptr()] = st.nbytes()
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = layer(src, pos, ref)
        saved[switch] = sum(seen.values())
        del out
    T = B * Hh * Hh
    print("saved bytes: without %d with %d" % (saved["0"], saved["1"]))
    assert saved["1"] <= saved["0"] - (T * d_ff + 2 * T * 256) + 64
