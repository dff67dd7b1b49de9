"""The training gradients of the BEV transformer's linears and LayerNorms on the GPU: `lss_linear_wgrad` and
`lss_layernorm_bwd` through the C ABI against fp64 with the derived bounds of tests/transformer_grad_ref.py (bit equality
for the exact weight-gradient cases), the autograd nodes `_LinearFn` / `_LayerNormFn`, and `TransformerEncoderLayer` on
the native route against the torch composition it replaces: parity through an fp64 middle, routing, the reference loop,
graph capture and peak memory.  Every test sets LSS_TRANSFORMER_NATIVE itself, so none depends on the switch's default.
"""
import copy
import ctypes

import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

import transformer_gemm_ref as R  # noqa: E402
import transformer_grad_ref as G  # noqa: E402
from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from lss2_multimodal_nu_amd import transformer_modules as tm  # noqa: E402

_id = lambda c: c.name  # noqa: E731
CANARY = -7.0          # exact in bf16 and fp32
DT = {torch.float32: ops.DT_F32, torch.bfloat16: ops.DT_BF16}
PAD_ROWS = 128         # rows of 1e4 behind x and dy: a whole stage, should a kernel read past T


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _padded(t, front=8):
    """t's rows inside a larger allocation: `front` elements and PAD_ROWS rows of 1e4 around them.  Returns (buffer,
    element offset of the tensor)."""
    cols = t.shape[1]
    buf = torch.full((front + (t.shape[0] + PAD_ROWS) * cols,), G.PAD_VALUE, dtype=t.dtype, device="cuda")
    buf[front:front + t.numel()] = t.reshape(-1).cuda()
    return buf, front


def _guarded(numel, dtype, off):
    """An output of `numel` elements inside a canary-filled allocation, `off` elements from its start."""
    return torch.full((numel + 2 * off + 64,), CANARY, dtype=dtype, device="cuda")


def _take(buf, off, shape):
    n = 1
    for s in shape:
        n *= s
    out = buf[off:off + n].clone().reshape(shape)
    rest = torch.cat([buf[:off], buf[off + n:]])
    assert bool((rest == CANARY).all()), "words around the output were written"
    return out


# ----------------------------------------------------------------------------------------------------------------------
# lss_linear_wgrad
# ----------------------------------------------------------------------------------------------------------------------
def run_wgrad(c, x, dy, want_dw=True, want_db=True):
    """Two calls through the C ABI on guarded buffers; returns (dw, db) of the first and asserts the second's bits."""
    xb, xo = _padded(x)
    db_, do = _padded(dy)
    nbytes = N.lib().lss_linear_wgrad_workspace_bytes(c.T, c.N, c.K)
    assert nbytes == G.wgrad_workspace_bytes(c.T, c.N, c.K)
    outs = []
    for fill in (0xFF, 0x00):   # the workspace's contents do not matter (0xFF..: NaNs)
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        wbuf, bbuf = _guarded(c.N * c.K, torch.float32, 32), _guarded(c.N, torch.float32, 3)
        rc = N.lib().lss_linear_wgrad(_vp(xb, xo), _vp(db_, do), c.T, c.N, c.K, _vp(ws), nbytes,
                                      _vp(wbuf, 32) if want_dw else None, _vp(bbuf, 3) if want_db else None, N.stream())
        N.check(rc, "lss_linear_wgrad")
        torch.cuda.synchronize()
        if not want_dw:
            assert bool((wbuf == CANARY).all())
        if not want_db:
            assert bool((bbuf == CANARY).all())
        outs.append((_take(wbuf, 32, (c.N, c.K)) if want_dw else None, _take(bbuf, 3, (c.N,)) if want_db else None))
    for a, b in zip(*outs):
        if a is not None:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls differ"
    return outs[0]


@pytest.mark.parametrize("exact", [False, True], ids=["randn", "exact"])
@pytest.mark.parametrize("c", G.WGRAD_CASES, ids=_id)
def test_linear_wgrad_against_fp64(c, exact, report):
    x, dy, ref = G.wgrad_case_data(c.name, exact)
    dw, db = run_wgrad(c, x, dy)
    e_w = G.check(dw, ref.dw, ref.bound_dw, c.name + ".dw")
    e_b = G.check(db, ref.db, ref.bound_db, c.name + ".db")
    report("linear_wgrad/%s/%s/dw_l2" % (c.name, "exact" if exact else "randn"), e_w[1])
    report("linear_wgrad/%s/%s/db_l2" % (c.name, "exact" if exact else "randn"), e_b[1])
    if exact:
        assert torch.equal(dw.double().cpu(), ref.dw) and torch.equal(db.double().cpu(), ref.db)


def test_the_split_case_spans_three_splits_with_a_ragged_last_one():
    c = G.WGRAD_BY_NAME["three_splits_ragged"]
    nbytes = N.lib().lss_linear_wgrad_workspace_bytes(c.T, c.N, c.K)
    splits = nbytes // (4 * (c.N * c.K + c.N))
    sp = G.wgrad_split(c.T, c.N, c.K)
    assert splits == sp.splits >= 3 and nbytes % (4 * (c.N * c.K + c.N)) == 0
    last = c.T - G.WG_TOK * sp.per * (sp.splits - 1)
    assert 0 < last < G.WG_TOK * sp.per and last % 32 != 0


@pytest.mark.parametrize("want", [(True, False), (False, True)], ids=["dw_only", "db_only"])
def test_linear_wgrad_one_output_only(want):
    c = G.WGRAD_BY_NAME["three_splits_ragged"]
    x, dy, ref = G.wgrad_case_data(c.name, True)
    dw, db = run_wgrad(c, x, dy, *want)
    if want[0]:
        assert db is None and torch.equal(dw.double().cpu(), ref.dw)
    else:
        assert dw is None and torch.equal(db.double().cpu(), ref.db)


def test_linear_wgrad_nan_reaches_its_own_row_only():
    c = G.WGRAD_BY_NAME["three_splits_ragged"]
    x, dy, _ = G.wgrad_case_data(c.name, True)
    t, n = 137, 5
    dz = dy.clone()
    dz[t, n] = 0.0
    ref = G.ref_wgrad(c, x, dz, True)
    dn = dy.clone()
    dn[t, n] = float("nan")
    dw, db = (t.cpu() for t in ops.linear_wgrad(x.cuda(), dn.cuda()))
    keep = torch.ones(c.N, dtype=torch.bool)
    keep[n] = False
    assert bool(torch.isnan(dw[n]).all()) and bool(torch.isnan(db[n]))
    assert torch.equal(dw[keep].double(), ref.dw[keep]) and torch.equal(db[keep].double(), ref.db[keep])


def test_linear_wgrad_wrapper_and_workspace_cache():
    c = G.WGRAD_BY_NAME["one_past_a_block"]
    x, dy, ref = G.wgrad_case_data(c.name, True)
    a = ops.linear_wgrad(x.cuda(), dy.cuda())
    b = ops.linear_wgrad(x.cuda(), dy.cuda())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0].double().cpu(), ref.dw) and torch.equal(a[1].double().cpu(), ref.db)
    assert ops.linear_wgrad(x.cuda(), dy.cuda(), want_db=False)[1] is None
    with pytest.raises(ValueError):
        ops.linear_wgrad(x.cuda()[:, :32].contiguous(), dy.cuda())


# ----------------------------------------------------------------------------------------------------------------------
# lss_layernorm_bwd
# ----------------------------------------------------------------------------------------------------------------------
def run_lnb(c, x, dy, gamma):
    xb, xo = _padded(x)
    gb, go = _padded(dy)
    odt = torch.bfloat16 if c.dx_bf16 else torch.float32
    nbytes = N.lib().lss_layernorm_bwd_workspace_bytes(c.rows)
    gm = gamma.cuda()
    outs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        dxb = _guarded(c.rows * G.C, odt, 8)
        dgb, dbb = _guarded(G.C, torch.float32, 5), _guarded(G.C, torch.float32, 1)
        rc = N.lib().lss_layernorm_bwd(_vp(xb, xo), DT[x.dtype], _vp(gb, go), DT[dy.dtype], _vp(gm), c.rows, G.C, G.EPS,
                                       _vp(ws), nbytes, _vp(dxb, 8), DT[odt], _vp(dgb, 5), _vp(dbb, 1), N.stream())
        N.check(rc, "lss_layernorm_bwd")
        torch.cuda.synchronize()
        outs.append((_take(dxb, 8, (c.rows, G.C)), _take(dgb, 5, (G.C,)), _take(dbb, 1, (G.C,))))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), "two calls differ"
    return outs[0]


@pytest.mark.parametrize("c", G.LNB_CASES, ids=_id)
def test_layernorm_bwd_against_fp64(c, report):
    for first in G.lnb_firsts(c):
        x, dy, gamma = G.make_lnb_inputs(c, first)
        ref = G.ref_layernorm_bwd(x, dy, gamma, G.EPS, c.dx_bf16)
        dx, dg, db = run_lnb(c, x, dy, gamma)
        assert dx.dtype == (torch.bfloat16 if c.dx_bf16 else torch.float32)
        e = G.check(dx, ref.dx, ref.bound_dx, "%s.%d.dx" % (c.name, first))
        G.check(dg, ref.dgamma, ref.bound_dgamma, "%s.%d.dgamma" % (c.name, first))
        G.check(db, ref.dbeta, ref.bound_dbeta, "%s.%d.dbeta" % (c.name, first))
        report("layernorm_bwd/%s/%d/dx_l2" % (c.name, first), e[1])


# ----------------------------------------------------------------------------------------------------------------------
# the nodes
# ----------------------------------------------------------------------------------------------------------------------
NODE_B, NODE_H, NODE_W = 2, 9, 14
LINEARS = [("offsets_logits", 192, 256, True), ("value_proj", 256, 256, True), ("output_proj", 256, 256, False),
           ("linear1", 1024, 256, False), ("linear2", 256, 1024, False)]


@pytest.mark.parametrize("name,Nout,K,out_f32", LINEARS, ids=[l[0] for l in LINEARS])
def test_linear_node_against_fp64_autograd(name, Nout, K, out_f32, report):
    g = R._gen("node_" + name)
    T = NODE_B * NODE_H * NODE_W
    x = torch.randn(NODE_B, NODE_H * NODE_W, K, generator=g)
    w = torch.randn(Nout, K, generator=g) / K ** 0.5
    b = torch.randn(Nout, generator=g)
    dy = 0.25 * torch.randn(NODE_B, NODE_H * NODE_W, Nout, generator=g)
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = tm._LinearFn.apply(xg, wg, bg, out_f32)
    assert y.dtype == (torch.float32 if out_f32 else torch.bfloat16) and tuple(y.shape) == tuple(dy.shape)
    y.backward(dy.cuda().to(y.dtype))
    assert (xg.grad.dtype, wg.grad.dtype, bg.grad.dtype) == (torch.float32,) * 3
    # fp64 autograd of F.linear on the bf16-rounded operands
    xb, wb, dyb = x.bfloat16(), w.bfloat16(), dy.bfloat16()
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (xb, wb, b))
    y64 = F.linear(x64, w64, b64)
    y64.backward(dyb.double())
    # forward and dx: the GEMM bound of transformer_gemm_ref; dw, db: the weight-gradient bound
    fc = R.GemmCase(name, NODE_B, NODE_H, NODE_W, K, Nout, False, True, False, R.ACT_NONE, out_f32, False, False)
    fwd = R.ref_gemm(fc, dict(x=xb.reshape(NODE_B, NODE_H, NODE_W, K), w=wb, scale=None, shift=b, residual=None))
    assert float((fwd.out.reshape(y64.shape) - y64.detach()).abs().max()) <= 1e-12 * float(y64.detach().abs().max())
    R.check(y, fwd.out.reshape(y64.shape), fwd.bound.reshape(y64.shape), name + ".y")
    bc = R.GemmCase(name + "_dx", NODE_B, NODE_H, NODE_W, Nout, K, False, False, False, R.ACT_NONE, False, False, False)
    bwd = R.ref_gemm(bc, dict(x=dyb.reshape(NODE_B, NODE_H, NODE_W, Nout), w=wb.t().contiguous(), scale=None, shift=None,
                              residual=None))
    assert float((bwd.out.reshape(x64.shape) - x64.grad).abs().max()) <= 1e-12 * float(x64.grad.abs().max())
    e = R.check(xg.grad, x64.grad, bwd.bound.reshape(x64.shape), name + ".dx")
    wc = G.WgradCase(name, T, Nout, K)
    ref = G.ref_wgrad(wc, xb.reshape(T, K), dyb.reshape(T, Nout), False)
    assert float((ref.dw - w64.grad).abs().max()) <= 1e-12 * float(w64.grad.abs().max())
    ew = G.check(wg.grad, w64.grad, ref.bound_dw, name + ".dw")
    G.check(bg.grad, b64.grad, ref.bound_db, name + ".db")
    report("linear_node/%s/dx_l2" % name, e[1])
    report("linear_node/%s/dw_l2" % name, ew[1])


@pytest.mark.parametrize("x_bf16", [False, True], ids=["x_f32", "x_bf16"])
def test_layernorm_node_against_fp64_autograd(x_bf16, report):
    g = R._gen("node_layernorm")
    x = torch.randn(NODE_B, NODE_H * NODE_W, G.C, generator=g) * 1.5 + 0.25
    x = x.bfloat16() if x_bf16 else x
    gamma, beta = R.make_ln_params(g)
    dy = torch.randn(NODE_B, NODE_H * NODE_W, G.C, generator=g)
    xg, gg, bg = (t.cuda().requires_grad_(True) for t in (x, gamma, beta))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = tm._LayerNormFn.apply(xg, gg, bg, G.EPS)
    assert y.dtype == torch.float32
    y.backward(dy.cuda())
    assert (xg.grad.dtype, gg.grad.dtype, bg.grad.dtype) == (x.dtype, torch.float32, torch.float32)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y64 = F.layer_norm(x64, (G.C,), g64, b64, G.EPS)
    y64.backward(dy.double())
    rows = NODE_B * NODE_H * NODE_W
    yr, yb = R.ref_layernorm(x.double().reshape(rows, G.C), 0.0, gamma, beta, G.EPS, False)
    R.check(y.reshape(rows, G.C), y64.detach().reshape(rows, G.C), yb, "ln.y")
    ref = G.ref_layernorm_bwd(x.reshape(rows, G.C), dy.reshape(rows, G.C), gamma, G.EPS, x_bf16)
    assert float((ref.dx - x64.grad.reshape(rows, G.C)).abs().max()) <= 1e-9
    e = G.check(xg.grad.reshape(rows, G.C), x64.grad.reshape(rows, G.C), ref.bound_dx, "ln.dx")
    G.check(gg.grad, g64.grad, ref.bound_dgamma, "ln.dgamma")
    G.check(bg.grad, b64.grad, ref.bound_dbeta, "ln.dbeta")
    report("layernorm_node/%s/dx_l2" % ("bf16" if x_bf16 else "f32"), e[1])


# ----------------------------------------------------------------------------------------------------------------------
# the layer
# ----------------------------------------------------------------------------------------------------------------------
def make_layer(seed, d_model=256, d_ff=1024, dropout=0.0):
    """Every parameter redrawn from the seed (`_reset_parameters` zeroes the offset and attention weights, which would
    leave their gradient paths trivial)."""
    layer = tm.TransformerEncoderLayer(d_model, 8, d_ff, dropout).train()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if name.startswith("norm") and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return layer


def layer_inputs(B, H, seed, d_model=256):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, H * H, d_model, generator=g)
    pos = tm.PositionEmbeddingSine(d_model // 2, normalize=True).table(H, H, "cpu")      # (H*H, d_model)
    pos = pos.t().reshape(1, d_model, H, H).expand(B, -1, -1, -1).contiguous()
    ref = tm.LightweightBEVTransformer.reference_points(H, H, "cpu").expand(B, -1, -1).contiguous()
    Gw = torch.randn(B, H * H, d_model, generator=g)
    return src, pos, ref, Gw


def run_layer(layer, inputs, monkeypatch, switch, amp=torch.bfloat16, device="cuda", expect=None):
    """One forward + backward; returns {name: CPU tensor} of the output, the input gradient and every parameter
    gradient.  expect: the route the counter must show."""
    src, pos, ref, Gw = (t.to(device) for t in inputs)
    if device == "cpu":
        src, pos, ref, Gw = src.double(), pos.double(), ref.double(), Gw.double()
    monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", switch)
    layer.zero_grad(set_to_none=True)
    src = src.clone().requires_grad_(True)
    before = dict(tm.TRANSFORMER_CALLS)
    with torch.autocast("cuda", dtype=amp or torch.bfloat16, enabled=amp is not None and device == "cuda"):
        out = layer(src, pos, ref)
    (out.to(Gw.dtype) * Gw).sum().backward()
    if expect is not None:
        other = "composition" if expect == "native" else "native"
        assert tm.TRANSFORMER_CALLS[expect] == before[expect] + 1 and tm.TRANSFORMER_CALLS[other] == before[other]
    res = {"out": out.detach().cpu(), "src.grad": src.grad.cpu()}
    for k, p in layer.named_parameters():
        res[k] = p.grad.detach().cpu().clone()
    return res


def rel_l2(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).norm() / ref.norm())


def test_layer_native_against_composition_through_fp64(monkeypatch, report):
    """B = 2, 12 x 12 tokens, dropout 0, every parameter redrawn.  The middle is the module's torch composition in fp64 on
    the CPU; for the output, the input gradient and every parameter gradient the native route's relative L2 distance to
    it is at most twice the composition's own (both under bf16 autocast on the GPU) plus 2^-9, half a bf16 ulp: both
    paths round at the same points.  The yardstick is the existing composition, not the new code.
    Measured (MI355X), relative L2 distance to the fp64 middle, composition / native:
      out 3.72e-3 / 3.37e-3          src.grad 5.23e-2 / 4.16e-2
      sampling_offsets.weight 9.36e-2 / 7.24e-2, .bias 9.05e-2 / 7.32e-2
      attention_weights.weight 1.11e-2 / 9.41e-3, .bias 1.14e-2 / 9.45e-3
      value_proj.weight 8.74e-3 / 7.50e-3, .bias 4.67e-3 / 4.14e-3
      output_proj.weight 8.55e-3 / 7.16e-3, .bias 3.92e-3 / 3.30e-3
      linear1.weight 5.83e-3 / 5.24e-3, .bias 4.98e-3 / 4.43e-3      linear2.weight 5.29e-3 / 4.74e-3, .bias 2.52e-3 / 1.76e-3
      norm1.weight 4.20e-3 / 3.74e-3, .bias 3.10e-3 / 2.82e-3        norm2.weight 3.65e-3 / 3.09e-3, .bias 8.49e-8 / 1.01e-7"""
    layer = make_layer(11)
    inputs = layer_inputs(2, 12, 12)
    mid = run_layer(copy.deepcopy(layer).double(), inputs, monkeypatch, "0", amp=None, device="cpu", expect="composition")
    gl = copy.deepcopy(layer).cuda()
    comp = run_layer(gl, inputs, monkeypatch, "0", expect="composition")
    nat = run_layer(gl, inputs, monkeypatch, "1", expect="native")
    assert nat["out"].dtype == comp["out"].dtype and nat["src.grad"].dtype == comp["src.grad"].dtype
    assert set(nat) == set(comp) == set(mid) and len(nat) == 2 + 16
    bad = []
    for k in sorted(mid):
        assert nat[k].dtype == comp[k].dtype, k
        dc, dn = rel_l2(comp[k], mid[k]), rel_l2(nat[k], mid[k])
        print("%-40s composition %.3e native %.3e" % (k, dc, dn))
        report("transformer_layer/%s/composition" % k, dc)
        report("transformer_layer/%s/native" % k, dn)
        if not dn <= 2.0 * dc + 2.0 ** -9:
            bad.append((k, dn, dc))
    assert not bad, bad


def test_native_route_runs_without_library_linear_or_layer_norm(monkeypatch):
    layer = make_layer(12).cuda()
    inputs = layer_inputs(1, 8, 13)

    def boom(*a, **k):
        raise AssertionError("library op on the native route")

    monkeypatch.setattr(torch.nn.functional, "linear", boom)
    monkeypatch.setattr(torch.nn.functional, "layer_norm", boom)
    res = run_layer(layer, inputs, monkeypatch, "1", expect="native")
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    assert all(float(v.abs().max()) > 0 for v in res.values())


# gradients that, with d_model = 128, pass through grid_sample's backward: it scatters the value gradient with float
# atomics, so the library does not repeat its own bits there (the native sampling node takes d_model = 256 only)
BEHIND_GRID_SAMPLE = ("src.grad", "self_attn.value_proj.weight", "self_attn.value_proj.bias")


@pytest.mark.parametrize("case", ["fp32", "fp16_autocast", "d_model_128", "switch_0"])
def test_other_cases_take_the_composition_unchanged(case, monkeypatch):
    """fp32 without autocast, fp16 autocast, d_model = 128 and the switch at 0: the composition counter advances, and the
    results with the switch at 1 equal the switch-off results bit for bit."""
    d_model = 128 if case == "d_model_128" else 256
    layer = make_layer(14, d_model=d_model, d_ff=256).cuda()
    inputs = layer_inputs(1, 8, 15, d_model)
    amp = {"fp32": None, "fp16_autocast": torch.float16}.get(case, torch.bfloat16)
    off = run_layer(layer, inputs, monkeypatch, "0", amp=amp, expect="composition")
    on = run_layer(layer, inputs, monkeypatch, "0" if case == "switch_0" else "1", amp=amp, expect="composition")
    for k in off:
        if case == "d_model_128" and k in BEHIND_GRID_SAMPLE:
            assert rel_l2(on[k], off[k]) <= 1e-5, k
        else:
            assert torch.equal(on[k], off[k]), k


def _loop(layer0, inputs, monkeypatch, seed):
    monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", "1")
    layer = copy.deepcopy(layer0).cuda()
    src, pos, ref, Gw = (t.cuda() for t in inputs)
    params = list(layer.parameters())
    start = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=1e-3)
    torch.manual_seed(seed)
    losses = []
    before = tm.TRANSFORMER_CALLS["native"]
    for _ in range(3):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = layer(src, pos, ref)
            loss = F.mse_loss(out.float(), Gw)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        opt.step()
        losses.append(float(loss))
    assert tm.TRANSFORMER_CALLS["native"] == before + 3
    moved = [not torch.equal(a, b.detach()) for a, b in zip(start, params)]
    return losses, moved


def test_reference_loop_under_autocast(monkeypatch):
    """Three steps of autocast(bf16) + clip_grad_norm_(10) + Adam on the layer with dropout 0.1 (torch's dropout, seeded):
    the losses are finite, every parameter moves, and a second run from the same seed reproduces the losses."""
    layer = make_layer(16, dropout=0.1)
    inputs = layer_inputs(2, 10, 17)
    l1, moved = _loop(layer, inputs, monkeypatch, 5)
    l2, _ = _loop(layer, inputs, monkeypatch, 5)
    print("losses", l1)
    assert all(v == v and abs(v) < float("inf") for v in l1)
    assert all(moved), [n for (n, _), m in zip(layer.named_parameters(), moved) if not m]
    assert l1 == l2


def _capture_and_replay(step, statics):
    """`_capture_and_replay` of test_vovnet_lift_grad_gpu.py: eager warm-up on a side stream, one captured step, three
    replays on refreshed static inputs, each compared bit for bit with an eager step on the same inputs."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    gen = torch.Generator().manual_seed(12)
    for r in range(3):
        with torch.no_grad():
            for s_ in statics:
                s_.copy_(torch.randn(s_.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in static_out]
        want = step()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), (r, i)


def test_capture_layer_replays_equal_eager(monkeypatch):
    """Forward + backward of the layer (dropout 0) on the native route, captured after three eager warm-up steps and
    replayed three times on refreshed static inputs: the output and every gradient equal the eager step's bit for bit."""
    monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", "1")
    layer = make_layer(18).cuda()
    src, pos, ref, Gw = (t.cuda() for t in layer_inputs(2, 12, 19))
    src.requires_grad_(True)
    leaves = [src] + list(layer.parameters())

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = layer(src, pos, ref)
        return (out,) + torch.autograd.grad((out * Gw).sum(), leaves)

    before = dict(tm.TRANSFORMER_CALLS)
    _capture_and_replay(step, (src,))
    assert tm.TRANSFORMER_CALLS["native"] == before["native"] + 3 + 1 + 3
    assert tm.TRANSFORMER_CALLS["composition"] == before["composition"]


def test_peak_memory_reported(monkeypatch, report):
    """Peak memory of one forward + backward at B = 2, 50 x 50, native and composition (second round each: workspaces
    are cached).  Reported, no threshold."""
    layer = make_layer(20).cuda()
    src, pos, ref, Gw = (t.cuda() for t in layer_inputs(2, 50, 21))
    src.requires_grad_(True)
    peak = {}
    for switch in ("1", "0", "1", "0"):
        monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", switch)
        layer.zero_grad(set_to_none=True)
        src.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = layer(src, pos, ref)
        (out * Gw).sum().backward()
        torch.cuda.synchronize()
        peak[switch] = torch.cuda.max_memory_allocated() - base
    print("peak bytes: native %d composition %d" % (peak["1"], peak["0"]))
    report("transformer_layer/peak_bytes/native", peak["1"])
    report("transformer_layer/peak_bytes/composition", peak["0"])
    assert peak["1"] > 0 and peak["0"] > 0
