"""The BEV transformer's deformable-attention core (`deform_attn_kernel` through `ops.deform_attn`, `ops.deform_attn_pts`
and the C entry `lss_deform_attn_fwd`) and `add_pos_kernel` alone against fp64.

References, cases, variants and bounds: tests/deform_attn_ref.py.  Every bound is DERIVED there (u, a count of operations,
magnitude sums and the local slope of the sampled map); nothing is taken from a kernel.  Every measured error is
`report`ed, with its largest error / bound ratio."""
import ctypes
import functools

import pytest
import torch

import deform_attn_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402

E_SHAPE, E_LAYOUT, E_ALIGN = -2, -3, -4
_id = lambda c: c.name  # noqa: E731
V = R.VARIANT_BY_NAME
SEL_VARIANTS = [v for v in R.VARIANTS if not v.bias and not v.pts]


def _p(t, offset_bytes=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset_bytes)


def _guarded(n, dtype):
    """A NaN-filled buffer of n elements with 256 bytes of sentinels on either side; returns (buffer, pad)."""
    pad = 256 // torch.empty(0, dtype=dtype).element_size()
    b = torch.full((pad + n + pad,), float("nan"), dtype=dtype, device="cuda")
    b[:pad] = 7.0
    b[pad + n:] = 7.0
    return b, pad


def _pads_ok(b, pad, n):
    return bool((b[:pad] == 7.0).all()) and bool((b[pad + n:] == 7.0).all())


def _sentinels_ok(b, pad, n):
    return _pads_ok(b, pad, n) and bool(torch.isfinite(b[pad:pad + n]).all())


def _untouched(b, pad, n):
    return _pads_ok(b, pad, n) and bool(torch.isnan(b[pad:pad + n]).all())


def _move_allocator():
    torch.empty(1 << 20, device="cuda").normal_()   # the next outputs land elsewhere


@functools.lru_cache(maxsize=None)
def _ref(name, kind, bf16, bias, pts):
    """The fp64 reference of a problem: computed once, shared by both layouts, never written to."""
    c = R.BY_NAME[name]
    v = next(x for x in R.VARIANTS if (x.bf16, x.bias, x.pts) == (bf16, bias, pts))
    ins = R.make_inputs(c, kind, v)
    return ins, R.ref_deform_attn(c, ins)


@functools.lru_cache(maxsize=None)
def _problem(name, kind, vname):
    c, v = R.BY_NAME[name], V[vname]
    ins, ref = _ref(name, kind, v.bf16, v.bias, v.pts)
    value = R.to_head_major(ins["value"]) if v.layout == "hm" else ins["value"]
    dev = {k: (None if ins[k] is None else ins[k].cuda()) for k in ("ol", "token_bias", "ref_x", "ref_y", "ref_pts")}
    dev["value"] = value.cuda()
    return c, v, ins, dev, ref


def _run(c, v, dev, value=None, ol=None, ref_pts=None):
    value = dev["value"] if value is None else value
    ol = dev["ol"] if ol is None else ol
    B, N = ol.shape[0], c.H * c.W
    if v.pts:
        pts = dev["ref_pts"] if ref_pts is None else ref_pts
        return ops.deform_attn_pts(value.reshape(B, N, 256), ol.reshape(B, N, 192), pts, c.H, c.W)
    return ops.deform_attn(value, ol, dev["ref_x"], dev["ref_y"], token_bias=dev["token_bias"])


def _ratio(got, ref):
    return float(((got.detach().double().cpu() - ref.out).abs() / ref.bound).max())


# ----------------------------------------------------------------------------------------------------------------------
# against fp64
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", R.VARIANTS, ids=_id)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_deform_attn_against_fp64(c, kind, v, report):
    _, _, ins, dev, ref = _problem(c.name, kind, v.name)
    got = _run(c, v, dev)
    assert got.dtype == (torch.bfloat16 if v.bf16 else torch.float32) and tuple(got.shape) == tuple(ref.out.shape)
    tag = "deform_attn_fwd.%s.%s.%s" % (c.name, kind, v.name)
    emax, el2 = R.check(got, ref.out, ref.bound, tag)
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    report(tag + ".bound_over_max", float(ref.bound.max() / ref.out.abs().max()))
    report(tag + ".error_over_bound", _ratio(got, ref))


@pytest.mark.parametrize("v", SEL_VARIANTS, ids=_id)
def test_selector_rows_are_value_rows_bit_for_bit(v):
    c, _, ins, dev, ref = _problem("full_blocks", "selector", v.name)
    got = _run(c, v, dev).cpu()
    want = R.selector_rows(c, ins)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(got.double(), ref.out)                 # the fp64 reference is exact here as well
    # the (token, head)s whose target lies inside the image return that pixel's value row verbatim
    pix, scale = R.selector_expectation(c, ins)
    b, t, h = (scale == 1.0).nonzero(as_tuple=True)
    assert len(b) > 100
    rows = ins["value"].reshape(c.B, c.H * c.W, 8, 32)
    assert torch.equal(got.reshape(c.B, c.H * c.W, 8, 32)[b, t, h], rows[b, pix[b, t, h], h])


@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_variants_agree(c, report):
    for kind in R.KINDS:
        run = lambda vname: _run(c, V[vname], _problem(c.name, kind, vname)[3])  # noqa: E731
        grid = run("nhwc_f32")
        assert torch.equal(run("pts_shared").reshape(grid.shape), grid)       # same arithmetic, same bits
        assert torch.equal(run("hm_f32"), grid)                                # the layout only moves addresses
        gb = run("nhwc_bf16")
        assert torch.equal(run("hm_bf16"), gb) and not torch.equal(gb.float(), grid)
        for dt in ("f32", "bf16"):
            nb, hb = run("nhwc_%s_bias" % dt), run("hm_%s_bias" % dt)
            assert torch.equal(nb, hb)
            # the bias form of the same problem: inside the bound of the undivided problem's reference, once the bound
            # is told of the fp32 rounding of the split (ol - bias)
            _, _, bins, _, _ = _problem(c.name, kind, "nhwc_%s_bias" % dt)
            full = _problem(c.name, kind, "nhwc_%s" % dt)[4]
            cross = R.ref_deform_attn(c, bins, input_err=R.U32 * bins["ol"].abs())
            tag = "deform_attn_fwd.%s.%s.bias_%s_vs_undivided" % (c.name, kind, dt)
            R.check(hb, full.out, cross.bound, tag)
            report(tag + ".error_over_bound", float(((hb.double().cpu() - full.out).abs() / cross.bound).max()))


# ----------------------------------------------------------------------------------------------------------------------
# stray writes, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["one_token", "odd_9", "odd_105_wide"])
def test_no_stray_writes(name, bf16):
    dt = "bf16" if bf16 else "f32"
    for vname in ("nhwc_%s" % dt, "hm_%s_bias" % dt, "hm_%s" % dt) + (() if bf16 else ("pts_shared", "pts_per_sample")):
        c, v, ins, dev, _ = _problem(name, "random", vname)
        n = c.B * c.H * c.W * 256
        buf, pad = _guarded(n, torch.bfloat16 if bf16 else torch.float32)
        keep = {k: t.clone() for k, t in dev.items() if t is not None}
        if v.pts:
            pts, rstride = ops._ref_pts_arg(dev["ref_pts"], c.B, c.H * c.W)
            assert rstride == (0 if v.pts == "shared" or c.B == 1 else 2 * c.H * c.W)
            rc = N.lib().lss_deform_attn_pts_fwd(_p(dev["value"]), _p(dev["ol"]), _p(pts), rstride, c.B, c.H, c.W, 8, 8, 256,
                                                 _p(buf, 256), N.stream())
        else:
            rc = N.lib().lss_deform_attn_fwd(_p(dev["value"]), ops.VALUE_HEAD_MAJOR if v.layout == "hm" else ops.VALUE_NHWC,
                                             _p(dev["ol"]), _p(dev["token_bias"]), _p(dev["ref_x"]), _p(dev["ref_y"]),
                                             c.B, c.H, c.W, 8, 8, 256, int(bf16), _p(buf, 256), N.stream())
        torch.cuda.synchronize()
        assert rc == 0 and _sentinels_ok(buf, pad, n), vname
        assert all(torch.equal(dev[k], t) for k, t in keep.items()), vname       # no input was written to
        assert torch.equal(buf[pad:pad + n], _run(c, v, dev).reshape(-1)), vname


def test_abi_codes():
    assert (ops.DT_F32, ops.DT_BF16, ops.VALUE_NHWC, ops.VALUE_HEAD_MAJOR) == (0, 1, 0, 1)


# ----------------------------------------------------------------------------------------------------------------------
# samples are independent; runs are reproducible
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd_105_wide", "tall"])
def test_samples_are_independent_and_runs_bit_equal(name):
    for vname in ("nhwc_f32", "hm_f32", "nhwc_bf16", "hm_bf16_bias", "pts_shared", "pts_per_sample"):
        c, v, ins, dev, _ = _problem(name, "random", vname)
        whole = _run(c, v, dev)
        for b in range(c.B):
            pts = dev["ref_pts"][b:b + 1] if v.pts == "per_sample" else None
            alone = _run(c, v, dev, value=dev["value"][b:b + 1], ol=dev["ol"][b:b + 1], ref_pts=pts)
            assert torch.equal(alone[0], whole[b]), (vname, b)
        _move_allocator()
        assert torch.equal(_run(c, v, dev), whole), vname


# ----------------------------------------------------------------------------------------------------------------------
# non-finite values
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["interior", "corner", "last_corner"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("vname", ["nhwc_f32", "hm_bf16"])
def test_non_finite_value_stays_with_its_samplers(vname, bad, where):
    """Positions keep off the bilinear kinks and the clamp edges and no weight is zero, so the fp64 composition and the
    kernel multiply the planted element by the same nonzero weights.  The kernel reads an out-of-image tap at a clamped
    index with weight 0: after the clamp of loc to [0, 1] that index is an in-image tap of the same point, so 0 * NaN
    adds no output to the set."""
    c, v, ins, dev, _ = _problem("wide", "nudged", vname)
    B, H, W = c.B, c.H, c.W
    b, y, x = {"interior": (1, 4, 6), "corner": (0, 0, 0), "last_corner": (1, H - 1, W - 1)}[where]
    ch = 3 * 32 + 5
    val = ins["value"].clone()
    val[b, y, x, ch] = bad
    pins = dict(ins, value=val)
    ref = R.ref_deform_attn(c, pins)
    want = R.grid_sample_composition(val.double().reshape(B, H * W, 256), ins["ol"].double().reshape(B, H * W, 192),
                                     R.grid_points(ins["ref_x"], ins["ref_y"]).double().expand(B, H * W, 2), H, W)
    nf = ~torch.isfinite(want.reshape(B, H, W, 256))
    assert 0 < int(nf.sum()) and torch.equal(nf, ~torch.isfinite(ref.out))
    got = _run(c, v, dev, value=(R.to_head_major(val) if v.layout == "hm" else val).cuda()).cpu()
    assert torch.equal(~torch.isfinite(got.float()), nf)
    assert bool((nf.nonzero()[:, 0] == b).all()) and bool((nf.nonzero()[:, 3] == ch).all())
    R.check(got[~nf], ref.out[~nf], ref.bound[~nf], "finite outputs beside a planted %r" % bad)


# ----------------------------------------------------------------------------------------------------------------------
# add_pos
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", R.ADD_POS_B)
@pytest.mark.parametrize("T", R.ADD_POS_ROWS)
def test_add_pos_bit_exact(T, B, bf16):
    x, pos = R.make_add_pos_inputs(T, B, bf16)
    want = R.ref_add_pos(x, pos)
    xd, pd = x.cuda(), pos.cuda()
    xk, pk = xd.clone(), pd.clone()
    n = B * T * 256
    buf, pad = _guarded(n, x.dtype)
    rc = N.lib().lss_add_pos_fwd(_p(xd), _p(pd), B, T, 256, int(bf16), _p(buf, 256), N.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _pads_ok(buf, pad, n)
    assert R.same_bits(xd, xk) and R.same_bits(pd, pk)
    got = buf[pad:pad + n].view(B, T, 256)
    assert got.dtype == want.dtype and R.same_bits(got, want)
    assert R.same_bits(ops.add_pos(xd, pd), want)
    assert int(torch.isnan(got).sum()) == int(torch.isnan(want).sum()) >= 3


# ----------------------------------------------------------------------------------------------------------------------
# refusals write nothing
# ----------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    c, v, ins, dev, _ = _problem("odd_9", "random", "hm_f32_bias")
    n = c.B * c.H * c.W * 256
    buf, pad = _guarded(n, torch.float32)
    roomy = torch.zeros(dev["token_bias"].numel() + 16, device="cuda")     # a bias 8 bytes off a 16-B boundary, in bounds
    assert roomy.data_ptr() % 16 == 0

    def call(tb=_p(dev["token_bias"]), layout=ops.VALUE_HEAD_MAJOR, nh=8, npt=8, C=256, dt=0, B=c.B, value=_p(dev["value"])):
        rc = N.lib().lss_deform_attn_fwd(value, layout, _p(dev["ol"]), tb, _p(dev["ref_x"]), _p(dev["ref_y"]), B, c.H, c.W,
                                         nh, npt, C, dt, _p(buf, 256), N.stream())
        torch.cuda.synchronize()
        return rc

    for kw, code in ((dict(tb=_p(roomy, 8)), E_ALIGN), (dict(tb=_p(roomy, 4)), E_ALIGN), (dict(layout=2), E_LAYOUT),
                     (dict(dt=2), E_LAYOUT), (dict(nh=4), E_SHAPE), (dict(npt=4), E_SHAPE), (dict(C=128), E_SHAPE),
                     (dict(B=0), E_SHAPE), (dict(value=None), -1)):
        rc = call(**kw)
        assert rc == code and _untouched(buf, pad, n), kw
        with pytest.raises(ValueError):
            N.check(rc, "lss_deform_attn_fwd")
    tb8 = roomy[2:2 + dev["token_bias"].numel()].view_as(dev["token_bias"])
    assert tb8.is_contiguous() and tb8.data_ptr() % 16 == 8
    with pytest.raises(ValueError):
        ops.deform_attn(dev["value"], dev["ol"], dev["ref_x"], dev["ref_y"], token_bias=tb8)
    assert call() == 0 and _sentinels_ok(buf, pad, n)             # the same call with nothing wrong runs

    x, pos = (t.cuda() for t in R.make_add_pos_inputs(5, 3, False))
    xr = torch.zeros(x.numel() + 16, device="cuda")
    q, qpad = _guarded(x.numel(), torch.float32)
    for args, code in (((_p(x), _p(pos), 3, 5, 128, 0), E_SHAPE), ((_p(x), _p(pos), 3, 0, 256, 0), E_SHAPE),
                       ((_p(x), _p(pos), 3, 5, 256, 2), E_LAYOUT), ((_p(xr, 8), _p(pos), 3, 5, 256, 0), E_ALIGN),
                       ((_p(x), _p(xr, 8), 3, 5, 256, 0), E_ALIGN)):
        rc = N.lib().lss_add_pos_fwd(*args, _p(q, 256), N.stream())
        torch.cuda.synchronize()
        assert rc == code and _untouched(q, qpad, x.numel()), args[2:]
        with pytest.raises(ValueError):
            N.check(rc, "lss_add_pos_fwd")
