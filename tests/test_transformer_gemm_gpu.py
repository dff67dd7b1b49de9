"""The BEV transformer's GEMM (`linear_mfma_kernel` through `ops.conv2d_nhwc`), fused FFN (`ops.ffn_fused`), fused output
projection (`ops.linear_res_ln`) and LayerNorm (`ops.layernorm`) kernels alone against fp64.

References, cases and bounds: tests/transformer_gemm_ref.py.  Every bound is DERIVED there (u, a count of operations and
a magnitude sum); nothing is taken from a kernel.  Every measured error is `report`ed."""
import ctypes
import functools

import pytest
import torch

import transformer_gemm_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402

E_SHAPE, E_LAYOUT, E_ALIGN = -2, -3, -4
_id = lambda c: c.name  # noqa: E731
LN_IDS = ["plain", "ln"]


def _cuda(d):
    return {k: (None if v is None else v.cuda()) for k, v in d.items()}


def _report(report, tag, emax, el2, bound, ref):
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    report(tag + ".bound_over_max", float(bound.max() / ref.abs().max()))


def _p(t, offset_bytes=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset_bytes)


def _guarded(n, dtype):
    """A NaN-filled buffer of n elements with 256 bytes of sentinels (64 floats) on either side; returns (buffer, pad)."""
    pad = 256 // torch.empty(0, dtype=dtype).element_size()
    b = torch.full((pad + n + pad,), float("nan"), dtype=dtype, device="cuda")
    b[:pad] = 7.0
    b[pad + n:] = 7.0
    return b, pad


def _sentinels_ok(b, pad, n):
    return bool((b[:pad] == 7.0).all()) and bool((b[pad + n:] == 7.0).all()) and bool(torch.isfinite(b[pad:pad + n]).all())


def _move_allocator():
    torch.empty(1 << 20, device="cuda").normal_()   # the next outputs land elsewhere


def test_abi_codes():
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_GELU) == (R.ACT_NONE, R.ACT_RELU, R.ACT_GELU)


# ----------------------------------------------------------------------------------------------------------------------
# the GEMM kernel
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemm(name):
    """Inputs, device copies and the reference of a case: computed once, shared, never written to."""
    c = R.GEMM_BY_NAME[name]
    ins = R.make_gemm_inputs(c)
    return c, _cuda(ins), R.ref_gemm(c, ins)


def _run_gemm(c, dev, head_major=None, out_f32=None):
    hm = c.head_major if head_major is None else head_major
    return ops.conv2d_nhwc(dev["x"], dev["w"].view(1, c.N, c.K), (1, 1), 1, 0, dev["scale"], dev["shift"], dev["residual"],
                           c.act, dt=ops.DT_BF16, out_f32=c.out_f32 if out_f32 is None else out_f32, head_major=hm)


@pytest.mark.parametrize("c", R.GEMM_CASES, ids=_id)
def test_gemm_against_fp64(c, report, monkeypatch):
    """stats=None sends the call to linear_mfma_kernel; LSS_CONV_DIRECT=1 sends the same call to the direct kernel.  Both
    are inside the same bound, and from K = 64 on (two summation orders; for the GELU cases two erf implementations)
    they differ in some bit: the first run was the GEMM kernel.  The bits compared are those of the fp32 output of the
    same call: a bf16 store rounds a last-bit fp32 difference away in all but about one element in 20 000 (at K = 64
    and N = 72 the two bf16 outputs ARE bit-equal), so it cannot tell the two kernels apart."""
    assert R.gemm_dispatch_ok(c)
    _, dev, ref = _gemm(c.name)
    got = _run_gemm(c, dev)
    assert got.dtype == (torch.float32 if c.out_f32 else torch.bfloat16) and tuple(got.shape) == tuple(ref.out.shape)
    tag = "transformer_gemm.linear_mfma." + c.name
    _report(report, tag, *R.check(got, ref.out, ref.bound, tag), ref.bound, ref.out)
    again = _run_gemm(c, dev)
    assert torch.equal(got, again)
    if c.head_major:
        return
    got32 = got if c.out_f32 else _run_gemm(c, dev, out_f32=True)
    monkeypatch.setenv("LSS_CONV_DIRECT", "1")
    direct = _run_gemm(c, dev)
    direct32 = direct if c.out_f32 else _run_gemm(c, dev, out_f32=True)
    monkeypatch.delenv("LSS_CONV_DIRECT")
    tag = "transformer_gemm.conv_direct." + c.name
    _report(report, tag, *R.check(direct, ref.out, ref.bound, tag), ref.bound, ref.out)
    assert got32.dtype == direct32.dtype == torch.float32
    if c.K >= 64:
        assert not torch.equal(got32, direct32)
        report("transformer_gemm.linear_mfma_vs_direct.%s.bf16_outputs_differing" % c.name,
               -1 if c.out_f32 else int((got != direct).sum()))
    assert torch.equal(_run_gemm(c, dev), got)   # and the GEMM kernel is back


def test_value_head_major_is_the_row_major_output_permuted():
    c, dev, ref = _gemm("value_head_major")
    hm, rm = _run_gemm(c, dev), _run_gemm(c, dev, head_major=False)
    HW = c.H * c.W
    assert tuple(hm.shape) == (c.B, c.N // 32, HW, 32) and tuple(rm.shape) == (c.B, c.H, c.W, c.N)
    assert torch.equal(hm.permute(0, 2, 1, 3).reshape(c.B, c.H, c.W, c.N), rm)
    assert torch.equal(hm, R.to_head_major(rm.reshape(c.B * HW, c.N), c.B, HW, c.N))


def test_gemm_two_runs_bit_equal():
    for name in ("k96_scalar_epilogue", "grid_12", "lin1_gelu_bf16"):
        c, dev, _ = _gemm(name)
        a = _run_gemm(c, dev)
        _move_allocator()
        assert torch.equal(a, _run_gemm(c, dev))


# ----------------------------------------------------------------------------------------------------------------------
# the fused FFN
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ffn(name):
    c = R.FFN_BY_NAME[name]
    ins = R.make_ffn_inputs(c)
    return c, _cuda(ins), R.ref_ffn(ins)


def _run_ffn(dev, ln, x=None):
    return ops.ffn_fused(dev["x"] if x is None else x, dev["w1"], dev["b1"], dev["w2"], dev["b2"],
                         ln=(dev["gamma"], dev["beta"], R.EPS) if ln else None)


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
@pytest.mark.parametrize("c", R.FFN_CASES, ids=_id)
def test_ffn_against_fp64(c, ln, report):
    _, dev, ref = _ffn(c.name)
    got = _run_ffn(dev, ln)
    assert tuple(got.shape) == (c.M, R.C) and got.dtype == (torch.bfloat16 if ln else torch.float32)
    want, bound = (ref.y_ln, ref.bound_ln) if ln else (ref.y, ref.bound)
    tag = "transformer_gemm.ffn_fused.%s.%s" % (c.name, LN_IDS[ln])
    _report(report, tag, *R.check(got, want, bound, tag), bound, want)
    report("transformer_gemm.ffn_fused.%s.ambiguous_share" % c.name, float(ref.ambiguous.double().mean()))
    if c.identity and not ln:
        # y - x is the sum of one or four hidden units: where none of them is ambiguous, their exact bf16 values and
        # the roundings of the adds - this is what tells an erf GELU from a tanh GELU inside the kernel
        clean = ref.clean
        assert float(clean.double().mean()) >= 0.9
        d = (got.double().cpu() - ref.y).abs()
        blocks = c.F // R.C
        hsum = R.bf16_rn(ref.h).abs().reshape(c.M, blocks, R.C).sum(1) + dev["x"].double().cpu().abs()
        assert bool((d[clean] <= ((blocks + 3) * R.U32 * hsum + R.TINY)[clean]).all())


@pytest.mark.parametrize("c", R.FFN_CASES, ids=_id)
def test_ffn_tail_is_the_layernorm_kernel_on_the_fp32_sum(c, report):
    """Both paths are two-pass LayerNorms of the same fp32 sums, so they agree bit for bit unless their two summation
    trees (32 lanes x 8 channels in the tail, 64 lanes x 4 in the row kernel) round a mean or a variance apart and that
    moves a bf16 rounding; where they do differ, both are inside the bound of the reference."""
    _, dev, ref = _ffn(c.name)
    fused = _run_ffn(dev, True)
    two = ops.layernorm(_run_ffn(dev, False), dev["gamma"], dev["beta"], R.EPS, torch.bfloat16)
    ndiff = int((fused != two).sum())
    report("transformer_gemm.ffn_fused.%s.tail_vs_layernorm_kernel.differing" % c.name, ndiff)
    if ndiff:
        R.check(fused, ref.y_ln, ref.bound_ln, "fused tail")
        R.check(two, ref.y_ln, ref.bound_ln, "layernorm kernel on the fp32 sum")


# ----------------------------------------------------------------------------------------------------------------------
# the fused output projection
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _proj(name):
    c = R.PROJ_BY_NAME[name]
    ins = R.make_proj_inputs(c)
    return c, _cuda(ins), R.ref_linear_res(ins, c.exact)


def _run_proj(dev, ln, x=None):
    return ops.linear_res_ln(dev["x"] if x is None else x, dev["w"], dev["bias"], dev["residual"],
                             ln=(dev["gamma"], dev["beta"], R.EPS) if ln else None)


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
@pytest.mark.parametrize("c", R.PROJ_CASES, ids=_id)
def test_linear_res_ln_against_fp64(c, ln, report):
    _, dev, ref = _proj(c.name)
    got = _run_proj(dev, ln)
    assert tuple(got.shape) == (c.M, R.C) and got.dtype == (torch.bfloat16 if ln else torch.float32)
    want, bound = (ref.y_ln, ref.bound_ln) if ln else (ref.y, ref.bound)
    tag = "transformer_gemm.linear_res_ln.%s.%s" % (c.name, LN_IDS[ln])
    _report(report, tag, *R.check(got, want, bound, tag), bound, want)


@pytest.mark.parametrize("c", R.PROJ_CASES, ids=_id)
def test_linear_res_ln_tail_is_the_layernorm_kernel_on_the_fp32_sum(c, report):
    """As for the FFN: bit-equal, or - where the two summation trees round apart - both inside the reference's bound."""
    _, dev, ref = _proj(c.name)
    fused = _run_proj(dev, True)
    two = ops.layernorm(_run_proj(dev, False), dev["gamma"], dev["beta"], R.EPS, torch.bfloat16)
    ndiff = int((fused != two).sum())
    report("transformer_gemm.linear_res_ln.%s.tail_vs_layernorm_kernel.differing" % c.name, ndiff)
    if ndiff:
        R.check(fused, ref.y_ln, ref.bound_ln, "fused tail")
        R.check(two, ref.y_ln, ref.bound_ln, "layernorm kernel on the fp32 sum")


# ----------------------------------------------------------------------------------------------------------------------
# the LayerNorm row kernel
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.LN_CASES, ids=_id)
def test_layernorm_against_fp64(c, report):
    out_dtype = torch.bfloat16 if c.out_bf16 else torch.float32
    for kind in R.LN_KINDS:
        x, gamma, beta = R.make_ln_inputs(c, kind)
        y, bound = R.ref_layernorm(x.double(), 0.0, gamma, beta, R.EPS, c.out_bf16)
        got = ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda(), R.EPS, out_dtype)
        assert got.dtype == out_dtype and tuple(got.shape) == (c.rows, R.C)
        tag = "transformer_gemm.layernorm.%s.%s" % (c.name, kind)
        _report(report, tag, *R.check(got, y, bound, tag), bound, y)
        if kind == "constant":   # 256 equal values: d = 0 in any summation tree, the output is beta exactly
            assert torch.equal(got.cpu(), beta.to(out_dtype).expand(c.rows, R.C))


# ----------------------------------------------------------------------------------------------------------------------
# stray writes: the outputs inside larger buffers, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------
def _call_ffn(dev, M, F, y, y_ln, x=None, d_model=R.C):
    g, b = (dev["gamma"], dev["beta"]) if y_ln is not None else (None, None)
    rc = N.lib().lss_ffn_fused_fwd(_p(dev["x"]) if x is None else x, _p(dev["w1"]), _p(dev["b1"]), _p(dev["w2"]), _p(dev["b2"]),
                                   M, d_model, F, y, _p(g), _p(b), R.EPS, y_ln, N.stream())
    torch.cuda.synchronize()
    return rc


def _call_proj(dev, M, y, y_ln, x=None, d_model=R.C):
    g, b = (dev["gamma"], dev["beta"]) if y_ln is not None else (None, None)
    rc = N.lib().lss_linear_res_ln_fwd(_p(dev["x"]) if x is None else x, _p(dev["w"]), _p(dev["bias"]), _p(dev["residual"]),
                                       M, d_model, y, _p(g), _p(b), R.EPS, y_ln, N.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
@pytest.mark.parametrize("name", ["f64_m1", "f128_m33", "f192_m129", "f1024_m257"])
def test_ffn_no_stray_writes(name, ln):
    c, dev, _ = _ffn(name)
    n = c.M * R.C
    buf, pad = _guarded(n, torch.bfloat16 if ln else torch.float32)
    out = _p(buf, 256)
    assert _call_ffn(dev, c.M, c.F, None if ln else out, out if ln else None, x=_p(dev["x"])) == 0
    assert _sentinels_ok(buf, pad, n)
    assert torch.equal(buf[pad:pad + n].view(c.M, R.C), _run_ffn(dev, ln))


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
@pytest.mark.parametrize("name", ["m127_randn", "m300_exact"])
def test_linear_res_ln_no_stray_writes(name, ln):
    c, dev, _ = _proj(name)
    n = c.M * R.C
    buf, pad = _guarded(n, torch.bfloat16 if ln else torch.float32)
    out = _p(buf, 256)
    assert _call_proj(dev, c.M, None if ln else out, out if ln else None, x=_p(dev["x"])) == 0
    assert _sentinels_ok(buf, pad, n)
    assert torch.equal(buf[pad:pad + n].view(c.M, R.C), _run_proj(dev, ln))


@pytest.mark.parametrize("rows", [1, 3, 5])
def test_layernorm_no_stray_writes(rows):
    for c in (x for x in R.LN_CASES if x.rows == rows):
        x, gamma, beta = (t.cuda() for t in R.make_ln_inputs(c, "unit"))
        out_dtype = torch.bfloat16 if c.out_bf16 else torch.float32
        n = rows * R.C
        buf, pad = _guarded(n, out_dtype)
        rc = N.lib().lss_layernorm_fwd(_p(x), int(c.in_bf16), _p(gamma), _p(beta), rows, R.C, R.EPS, _p(buf, 256),
                                       int(c.out_bf16), N.stream())
        torch.cuda.synchronize()
        assert rc == 0 and _sentinels_ok(buf, pad, n)
        assert torch.equal(buf[pad:pad + n].view(rows, R.C), ops.layernorm(x, gamma, beta, R.EPS, out_dtype))


# ----------------------------------------------------------------------------------------------------------------------
# rows are independent; runs are reproducible
# ----------------------------------------------------------------------------------------------------------------------
def _assert_only_row_changed(clean, dirty, row):
    assert not bool(torch.isfinite(dirty[row].float()).any())
    dirty = dirty.clone()
    dirty[row] = clean[row]
    assert torch.equal(dirty, clean)


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
@pytest.mark.parametrize("row", [5, 256], ids=["full_tile", "partial_tile"])
def test_ffn_rows_are_independent(row, ln):
    c, dev, _ = _ffn("f1024_m257")
    clean = _run_ffn(dev, ln)
    x = dev["x"].clone()
    x[row, 77] = float("nan")
    _assert_only_row_changed(clean, _run_ffn(dev, ln, x=x), row)


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
@pytest.mark.parametrize("row", [7, 299], ids=["full_tile", "partial_tile"])
def test_linear_res_ln_rows_are_independent(row, ln):
    c, dev, _ = _proj("m300_randn")
    clean = _run_proj(dev, ln)
    x = dev["x"].clone()
    x[row, 201] = float("nan")
    _assert_only_row_changed(clean, _run_proj(dev, ln, x=x), row)


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
def test_fused_kernels_two_runs_bit_equal(ln):
    _, fdev, _ = _ffn("f1024_m257")
    _, pdev, _ = _proj("m300_randn_offset50")
    a, b = _run_ffn(fdev, ln), _run_proj(pdev, ln)
    _move_allocator()
    assert torch.equal(a, _run_ffn(fdev, ln)) and torch.equal(b, _run_proj(pdev, ln))
    c = R.LN_CASES[-1]
    x, gamma, beta = (t.cuda() for t in R.make_ln_inputs(c, "offset_1000"))
    y = ops.layernorm(x, gamma, beta, R.EPS, torch.bfloat16 if ln else torch.float32)
    _move_allocator()
    assert torch.equal(y, ops.layernorm(x, gamma, beta, R.EPS, torch.bfloat16 if ln else torch.float32))


# ----------------------------------------------------------------------------------------------------------------------
# refusals write nothing
# ----------------------------------------------------------------------------------------------------------------------
def _refusal_operands(M, Dm, F):
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    Fa = max(F, 64)   # d_ff = 0 still needs live pointers
    return _cuda(dict(x=mk(M, Dm).bfloat16(), w1=mk(Fa, Dm).bfloat16(), b1=mk(Fa), w2=mk(Dm, Fa).bfloat16(), b2=mk(Dm),
                      w=mk(Dm, Dm).bfloat16(), bias=mk(Dm), residual=mk(M, Dm).bfloat16(), gamma=mk(Dm), beta=mk(Dm)))


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
@pytest.mark.parametrize("Dm,F", [(256, 0), (256, 32), (256, 96), (256, 1088), (128, 64)],
                         ids=["d_ff0", "d_ff32", "d_ff96", "d_ff1088", "d_model128"])
def test_ffn_refused_shapes_write_nothing(Dm, F, ln):
    M = 130
    dev = _refusal_operands(M, Dm, F)
    out = torch.full((2 * 128 * 256,), 7.0, dtype=torch.bfloat16 if ln else torch.float32, device="cuda")
    rc = _call_ffn(dev, M, F, None if ln else _p(out), _p(out) if ln else None, x=_p(dev["x"]), d_model=Dm)
    assert rc == E_SHAPE and bool((out == 7.0).all())
    with pytest.raises(ValueError):
        N.check(rc, "lss_ffn_fused_fwd")
    if F:
        with pytest.raises(ValueError):
            ops.ffn_fused(dev["x"], dev["w1"][:F].contiguous(), dev["b1"][:F].contiguous(),
                          dev["w2"][:, :F].contiguous(), dev["b2"], ln=(dev["gamma"], dev["beta"], R.EPS) if ln else None)
    if Dm != R.C:
        rc = _call_proj(dev, M, None if ln else _p(out), _p(out) if ln else None, x=_p(dev["x"]), d_model=Dm)
        assert rc == E_SHAPE and bool((out == 7.0).all())
        with pytest.raises(ValueError):
            ops.linear_res_ln(dev["x"], dev["w"], dev["bias"], dev["residual"],
                              ln=(dev["gamma"], dev["beta"], R.EPS) if ln else None)


@pytest.mark.parametrize("ln", [False, True], ids=LN_IDS)
def test_misaligned_x_is_refused_and_writes_nothing(ln):
    M = 130
    dev = _refusal_operands(M + 1, R.C, 64)
    out = torch.full((2 * 128 * 256,), 7.0, dtype=torch.bfloat16 if ln else torch.float32, device="cuda")
    y, y_ln = (None, _p(out)) if ln else (_p(out), None)
    assert _call_ffn(dev, M, 64, y, y_ln, x=_p(dev["x"], 8)) == E_ALIGN and bool((out == 7.0).all())
    assert _call_proj(dev, M, y, y_ln, x=_p(dev["x"], 8)) == E_ALIGN and bool((out == 7.0).all())
    x8 = dev["x"].view(-1)[4:4 + M * R.C].view(M, R.C)    # 4 bf16 elements = 8 bytes in
    assert x8.is_contiguous() and x8.data_ptr() % 16 == 8
    lnarg = (dev["gamma"], dev["beta"], R.EPS) if ln else None
    with pytest.raises(ValueError):
        ops.ffn_fused(x8, dev["w1"], dev["b1"], dev["w2"], dev["b2"], ln=lnarg)
    with pytest.raises(ValueError):
        ops.linear_res_ln(x8, dev["w"], dev["bias"], dev["residual"][:M], ln=lnarg)


def test_layernorm_refusals_write_nothing():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(8, 256, generator=g).cuda()
    gamma, beta = torch.randn(256, generator=g).cuda(), torch.randn(256, generator=g).cuda()
    out = torch.full((8 * 256,), 7.0, device="cuda")
    for rows, Cc in ((16, 128), (0, 256)):
        rc = N.lib().lss_layernorm_fwd(_p(x), 0, _p(gamma), _p(beta), rows, Cc, R.EPS, _p(out), 0, N.stream())
        torch.cuda.synchronize()
        assert rc == E_SHAPE and bool((out == 7.0).all())
        with pytest.raises(ValueError):
            N.check(rc, "lss_layernorm_fwd")
    with pytest.raises(ValueError):
        ops.layernorm(x.view(16, 128), gamma[:128].contiguous(), beta[:128].contiguous(), R.EPS, torch.float32)
    with pytest.raises(ValueError):
        ops.layernorm(x[:0], gamma, beta, R.EPS, torch.float32)


def test_head_major_needs_the_gemm_kernel():
    """Cout = 48 is below the GEMM kernel's 64: the call would fall to the direct kernel, which cannot write that layout."""
    g = torch.Generator().manual_seed(5)
    B, H, W, K, Cout = 2, 3, 5, 64, 48
    x = torch.randn(B, H, W, K, generator=g).bfloat16().cuda()
    w = torch.randn(1, Cout, K, generator=g).bfloat16().cuda()
    out = torch.full((B * H * W * 64,), 7.0, dtype=torch.bfloat16, device="cuda")
    rc = N.lib().lss_conv2d_fwd(_p(x), None, _p(w), None, None, None, _p(out), None, B, H, W, K, 0, 1, Cout, 1, 1, 1, 0,
                                ops.OUT_HEAD_MAJOR32, ops.DT_BF16, N.stream())
    torch.cuda.synchronize()
    assert rc == E_LAYOUT and bool((out == 7.0).all())
    with pytest.raises(ValueError):
        ops.conv2d_nhwc(x, w, (1, 1), 1, 0, head_major=True)
    y = ops.conv2d_nhwc(x, w, (1, 1), 1, 0)   # the same call without the layout runs (on the direct kernel)
    assert tuple(y.shape) == (B, H, W, Cout) and bool(torch.isfinite(y.float()).all())
