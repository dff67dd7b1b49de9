"""The deformable-attention backward alone (csrc/deform_grad.hip: deform_grad_ol_kernel, deform_absmax_kernel,
deform_scatter_kernel, deform_convert_kernel, through `ops.deform_attn_bwd` and the C entry `lss_deform_attn_bwd`) against
fp64.

Reference, cases, kinds and bounds: tests/deform_attn_grad_ref.py.  Every bound is DERIVED there (u, counts of operations,
magnitude sums, the forward helper's softmax and position errors, the fixed-point step); nothing is taken from a kernel.
Every other assertion here is an exact equality or one of the stated counts.  Every measured error is `report`ed with its
largest error / bound ratio."""
import ctypes
import functools

import pytest
import torch

import deform_attn_grad_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402

E_SHAPE, E_ALIGN, E_WORKSPACE = -2, -4, -5
_id = lambda c: c.name  # noqa: E731
IN_KEYS = ("value", "ol", "ref_pts", "d_out")


def _p(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes)


def _guarded(n, dtype):
    """A NaN-filled buffer of n elements (bytes of 0xFF for uint8) with 256 bytes of sentinels on either side."""
    pad = 256 // torch.empty(0, dtype=dtype).element_size()
    fill = 255 if dtype == torch.uint8 else float("nan")
    b = torch.full((pad + n + pad,), fill, dtype=dtype, device="cuda")
    b[:pad] = 7
    b[pad + n:] = 7
    assert (b.data_ptr() + 256) % 16 == 0
    return b, pad


def _pads_ok(b, pad, n):
    return bool((b[:pad] == 7).all()) and bool((b[pad + n:] == 7).all())


def _untouched(b, pad, n):
    body = b[pad:pad + n]
    return _pads_ok(b, pad, n) and bool(((body == 255) if b.dtype == torch.uint8 else torch.isnan(body)).all())


@functools.lru_cache(maxsize=None)
def _problem(name, kind, pts):
    """(case, inputs, their device copies, the fp64 reference): computed once, shared, never written to."""
    c = R.BY_NAME[name]
    ins = R.make_grad_inputs(c, kind, pts)
    return c, ins, {k: ins[k].cuda() for k in IN_KEYS}, R.ref_deform_grad(c, ins)


def _run(c, dev, **over):
    a = dict(dev, **over)
    return ops.deform_attn_bwd(a["value"], a["ol"], a["ref_pts"], a["d_out"], c.H, c.W)


def _check3(got_v, got_o, ref, tag, report=None):
    """The elementwise check of d_value, of the offsets part and of the logits part of d_ol."""
    parts = (("d_value", got_v, ref.d_value, ref.bound_value),
             ("d_offsets", got_o[..., :128], ref.d_ol[..., :128], ref.bound_ol[..., :128]),
             ("d_logits", got_o[..., 128:], ref.d_ol[..., 128:], ref.bound_ol[..., 128:]))
    for name, got, want, bound in parts:
        emax, el2 = R.check(got, want, bound, tag + "." + name)
        if report is not None:
            report("%s.%s.max" % (tag, name), emax)
            report("%s.%s.l2" % (tag, name), el2)
            report("%s.%s.bound_over_max" % (tag, name), float(bound.max() / want.abs().max().clamp_min(R.TINY)))
            report("%s.%s.error_over_bound" % (tag, name), R.error_over_bound(got, want, bound))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# against fp64
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", R.PTS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", R.GCASES, ids=_id)
def test_backward_against_fp64(c, kind, pts, report):
    _, ins, dev, ref = _problem(c.name, kind, pts)
    dv, do = _run(c, dev)
    assert dv.dtype == do.dtype == torch.float32
    assert tuple(dv.shape) == (c.B, c.H * c.W, 256) and tuple(do.shape) == (c.B, c.H * c.W, 192)
    _check3(dv, do, ref, "deform_attn_bwd.%s.%s.%s" % (c.name, kind, pts), report)


@pytest.mark.parametrize("pts", R.PTS)
@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_exact_kind_bit_for_bit(name, pts):
    """Kinks, clamp edges, out-of-image targets and weights of exactly 1/2: every fp32 operation is exact."""
    c, ins, dev, ref = _problem(name, "exact", pts)
    dv, do = (t.cpu() for t in _run(c, dev))
    assert torch.equal(dv, ref.d_value.float()) and torch.equal(dv.double(), ref.d_value.float().double())
    assert torch.equal(do, ref.d_ol.float())
    on_edge, outside = R.exact_edge_sets(c, ins)
    dox = do[..., :128].reshape(c.B, c.H * c.W, 8, 8, 2)
    assert int(outside.sum()) > 100 and bool((dox[outside] == 0).all())                 # mask 0
    # mask 1 at raw == 0 and raw == 1 exactly: non-zero wherever the integer dots do not cancel, which is most of them
    want = ref.d_ol[..., :128].reshape(dox.shape)[on_edge] != 0
    assert torch.equal(dox[on_edge] != 0, want) and int(want.sum()) * 2 > int(on_edge.sum()) > 100


@pytest.mark.parametrize("c", R.GCASES, ids=_id)
def test_shared_and_expanded_reference_points_give_the_same_bits(c):
    _, ins, dev, _ = _problem(c.name, "random", "shared")
    assert ins["ref_pts"].shape[0] == 1
    stride0 = dev["ref_pts"].expand(c.B, -1, -1)
    assert c.B == 1 or ops._ref_pts_arg(stride0, c.B, c.H * c.W)[1] == 0
    full = stride0.contiguous()
    assert ops._ref_pts_arg(full, c.B, c.H * c.W)[1] == (0 if c.B == 1 else 2 * c.H * c.W)
    dv0, do0 = _run(c, dev, ref_pts=stride0)
    dv1, do1 = _run(c, dev, ref_pts=full)
    dv2, do2 = _run(c, dev)
    assert torch.equal(dv0, dv1) and torch.equal(do0, do1) and torch.equal(dv0, dv2) and torch.equal(do0, do2)


# ----------------------------------------------------------------------------------------------------------------------
# the fixed point
# ----------------------------------------------------------------------------------------------------------------------
def test_zero_sample():
    c, ins, dev, _ = _problem("tiles_2x3", "random", "shared")
    dv0, do0 = _run(c, dev)
    d_out = dev["d_out"].clone()
    d_out[1] = 0.0
    dv, do = _run(c, dev, d_out=d_out)
    assert bool((_bits(dv[1]) == 0).all())                      # +0.0 everywhere: no NaN, no -0.0
    assert bool((do[1] == 0).all())
    assert torch.equal(_bits(dv[0]), _bits(dv0[0])) and torch.equal(_bits(do[0]), _bits(do0[0]))


@pytest.mark.parametrize("ch", [76, 77, 78, 79])      # each of the four positions of a 16-byte load of the abs-max pass
def test_outlier_in_one_sample(ch, report):
    c, ins, dev, ref0 = _problem("tiles_2x3", "random", "shared")
    dv0, do0 = _run(c, dev)
    d_out = ins["d_out"].clone()
    d_out[1, 300, ch] = 2.0 ** 20 * float(d_out.abs().max())
    ref = R.ref_deform_grad(c, ins, d_out=d_out)
    assert R.fx_exponents(d_out)[1] == R.fx_exponents(ins["d_out"])[1] + 20            # that sample's step grew 2^20-fold
    assert torch.equal(ref.bound_value[0], ref0.bound_value[0])
    dv, do = _run(c, dev, d_out=d_out.cuda())
    _check3(dv, do, ref, "deform_attn_bwd.tiles_2x3.outlier_ch%d" % ch, report)
    assert torch.equal(_bits(dv[0]), _bits(dv0[0])) and torch.equal(_bits(do[0]), _bits(do0[0]))
    assert not torch.equal(dv[1], dv0[1])                                               # small elements were flushed


@pytest.mark.parametrize("k", [-60, 60])
def test_power_of_two_scaling(k):
    c, ins, dev, _ = _problem("tiles_2x3", "random", "shared")
    dv0, do0 = _run(c, dev)
    dv, do = _run(c, dev, d_out=dev["d_out"] * 2.0 ** k)
    want_v, want_o = dv0 * 2.0 ** k, do0 * 2.0 ** k
    assert bool(torch.isfinite(want_v).all()) and bool(torch.isfinite(want_o).all())
    assert bool(((want_v != 0) == (dv0 != 0)).all()) and bool(((want_o != 0) == (do0 != 0)).all())   # nothing underflows
    assert torch.equal(_bits(dv), _bits(want_v)) and torch.equal(_bits(do), _bits(want_o))


def test_concentration_past_the_cap_of_F(report):
    """N = 8192: F = 49.  Every token adds (2 - 2^-23) 2^48 to the 256 sums of one cell: 2^62 - 2^38 in all, the largest
    sum the file comment's argument allows for d_out below 2."""
    c = R.Case("concentration", 1, 128, 64)
    Ntok = c.H * c.W
    cx, cy = 37, 101
    assert R.fx_bits(Ntok) == 49
    g = torch.Generator().manual_seed(49)
    lg = torch.full((1, Ntok, 8, 8), -200.0)
    lg[..., 0] = 0.0
    ins = dict(value=torch.randn(1, Ntok, 256, generator=g),
               ol=torch.cat([torch.zeros(1, Ntok, 128), lg.reshape(1, Ntok, 64)], -1),
               ref_pts=torch.tensor([(cx + 0.5) / 64, (cy + 0.5) / 128]).expand(1, Ntok, 2).contiguous(),
               d_out=torch.full((1, Ntok, 256), 2.0 - 2.0 ** -23))
    assert float(ins["d_out"][0, 0, 0]) == 2.0 - 2.0 ** -23 and R.fx_exponents(ins["d_out"]) == [1]
    dv, do = ops.deform_attn_bwd(*(ins[k].cuda() for k in IN_KEYS), c.H, c.W)
    want = torch.zeros(1, Ntok, 256)
    want[0, cy * c.W + cx] = 2.0 ** 14 - 2.0 ** -10
    assert float(want[0, cy * c.W + cx, 0]) == 8192 * (2.0 - 2.0 ** -23)                # 24 bits: an fp32 number
    assert torch.equal(dv.cpu(), want)
    assert bool((do == do[:, :1]).all())                                                # every token has the same problem
    tok = torch.arange(0, Ntok, 127)
    ref = R.ref_deform_grad(c, ins, tokens=tok)
    sub = do.cpu()[:, tok]
    for name, sl in (("d_offsets", slice(0, 128)), ("d_logits", slice(128, 192))):
        R.check(sub[..., sl], ref.d_ol[..., sl], ref.bound_ol[..., sl], "concentration." + name)
        report("deform_attn_bwd.concentration.%s.error_over_bound" % name,
               R.error_over_bound(sub[..., sl], ref.d_ol[..., sl], ref.bound_ol[..., sl]))


# ----------------------------------------------------------------------------------------------------------------------
# stray writes, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------
def _abi_call(c, dev, ws, dvb, dob, ws_bytes, pts=None, rstride=None, nh=8, npt=8, C=256, d_out=None):
    if pts is None:
        pts, rstride = ops._ref_pts_arg(dev["ref_pts"], c.B, c.H * c.W)
    rc = N.lib().lss_deform_attn_bwd(_p(dev["value"]), _p(dev["ol"]), _p(pts), rstride,
                                     _p(dev["d_out"]) if d_out is None else d_out, c.B, c.H, c.W, nh, npt, C, _p(ws, 256),
                                     ws_bytes, _p(dvb, 256), _p(dob, 256), N.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("pts", R.PTS)
@pytest.mark.parametrize("name", ["one_token", "odd_9", "odd_105_wide", "very_wide"])
def test_no_stray_writes(name, pts):
    c, ins, dev, _ = _problem(name, "random", pts)
    rows = c.B * c.H * c.W
    nbytes = N.lib().lss_deform_attn_bwd_workspace_bytes(c.B, c.H, c.W)
    assert nbytes == c.H * c.W * (256 * 8 + 8 * 4) + c.B * 4
    ws, wpad = _guarded(nbytes, torch.uint8)                     # exactly the bytes the entry asks for
    dvb, vpad = _guarded(rows * 256, torch.float32)
    dob, opad = _guarded(rows * 192, torch.float32)
    keep = {k: t.clone() for k, t in dev.items()}
    rc = _abi_call(c, dev, ws, dvb, dob, nbytes)
    assert rc == 0
    assert _pads_ok(ws, wpad, nbytes) and _pads_ok(dvb, vpad, rows * 256) and _pads_ok(dob, opad, rows * 192)
    got_v, got_o = dvb[vpad:vpad + rows * 256], dob[opad:opad + rows * 192]
    assert bool(torch.isfinite(got_v).all()) and bool(torch.isfinite(got_o).all())
    assert all(torch.equal(_bits(dev[k]), _bits(t)) for k, t in keep.items())            # no input was written to
    dv, do = _run(c, dev)
    assert torch.equal(_bits(got_v), _bits(dv).reshape(-1)) and torch.equal(_bits(got_o), _bits(do).reshape(-1))


def test_refused_calls_write_nothing():
    c, ins, dev, _ = _problem("odd_9", "random", "per_sample")
    rows = c.B * c.H * c.W
    nbytes = N.lib().lss_deform_attn_bwd_workspace_bytes(c.B, c.H, c.W)
    ws, wpad = _guarded(nbytes, torch.uint8)
    dvb, vpad = _guarded(rows * 256, torch.float32)
    dob, opad = _guarded(rows * 192, torch.float32)
    roomy = torch.zeros(rows * 256 + 16, device="cuda")          # a d_out 4 bytes off a 16-B boundary, in bounds
    assert roomy.data_ptr() % 16 == 0
    pts, rstride = ops._ref_pts_arg(dev["ref_pts"], c.B, c.H * c.W)
    for kw, code in ((dict(nh=4), E_SHAPE), (dict(C=128), E_SHAPE), (dict(d_out=_p(roomy, 4)), E_ALIGN),
                     (dict(pts=pts, rstride=2 * c.H * c.W + 1), E_ALIGN), (dict(ws_bytes=nbytes - 1), E_WORKSPACE)):
        rc = _abi_call(c, dev, ws, dvb, dob, **dict(dict(ws_bytes=nbytes), **kw))
        assert rc == code, (kw, rc)
        assert _untouched(ws, wpad, nbytes) and _untouched(dvb, vpad, rows * 256) and _untouched(dob, opad, rows * 192), kw
        with pytest.raises(ValueError):
            N.check(rc, "lss_deform_attn_bwd")
    assert _abi_call(c, dev, ws, dvb, dob, nbytes) == 0          # the same call with nothing wrong runs
    assert _pads_ok(dvb, vpad, rows * 256) and bool(torch.isfinite(dvb[vpad:vpad + rows * 256]).all())
