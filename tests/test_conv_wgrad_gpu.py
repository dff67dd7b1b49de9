"""The backward half of BevEncode's convs alone, per element, against fp64: K9w (csrc/conv_wgrad.hip: conv_wgrad_kernel
<3,3,-1,1> and the two launches of the 4x4-tap form), the split-order reduction, the GEMM fallback, the stride-2 forms
over phase planes, and the materialised upsample + concat with its adjoint (csrc/conv_grad.hip).

References, cases, bounds, the launch plan each case must reach and the planted errors: tests/conv_wgrad_ref.py.  The
exact cases (integer / dyadic operands) must equal the fp64 value bit for bit - an fp32 sum of small integers is exact
in any order, so one dropped, doubled or misplaced term of a sum over B H W positions shows at any shape and any
split; the bound cases must lie inside an elementwise bound DERIVED there.  Nothing is taken from a kernel.  Every
measured error of a bound case is `report`ed under conv_wgrad.*."""
import pytest
import torch

import conv_wgrad_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import modules as M  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402

_id = lambda c: c.name  # noqa: E731
_dev = lambda t: t.bfloat16().cuda()  # noqa: E731


def _assert_equal(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got.double() != want.double()).nonzero()   # (a NaN differs from everything)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ from the exact reference; first at %s: got %r want %r; all "
                             "differing positions span %s .. %s" % (what, bad.shape[0], got.numel(), i, float(got[i]),
                                                                    float(want[i]), bad.amin(0).tolist(), bad.amax(0).tolist()))


def _report(report, tag, emax, el2, bound, ref):
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    report(tag + ".bound_over_max", float(bound.max() / ref.abs().max()))


@pytest.fixture
def splits(monkeypatch):
    """Sets LSS_WGRAD_SPLITS (and LSS_WGRAD_DIRECT) for one case; the cached workspaces are keyed by shape alone, so they
    are dropped around every change of a switch that changes their size."""
    def set_(c_splits, direct=None):
        ops._wgrad_ws.clear()
        monkeypatch.delenv("LSS_WGRAD_SPLITS", raising=False)
        monkeypatch.delenv("LSS_WGRAD_DIRECT", raising=False)
        if c_splits is not None:
            monkeypatch.setenv("LSS_WGRAD_SPLITS", str(c_splits))
        if direct is not None:
            monkeypatch.setenv("LSS_WGRAD_DIRECT", direct)
    yield set_
    monkeypatch.delenv("LSS_WGRAD_SPLITS", raising=False)
    monkeypatch.delenv("LSS_WGRAD_DIRECT", raising=False)
    ops._wgrad_ws.clear()


def _library_nsplit(c):
    lib = ops.N.lib()
    if c.taps == 3:
        nbytes, per = lib.lss_conv2d_wgrad_workspace_bytes(c.B, c.H, c.W, c.Cin, c.Cout), 9 * c.Cout * c.Cin * 4
    else:
        nbytes, per = lib.lss_conv2d_wgrad4x4_workspace_bytes(c.B, c.H, c.W, c.Cin, c.Cout), 16 * c.Cout * c.Cin * 4
    assert nbytes > 0 and nbytes % per == 0, (c.name, nbytes, per)   # a tile is a multiple of 256 bytes: no rounding
    return nbytes // per


def _fill_workspaces_with_nans():
    assert ops._wgrad_ws
    for ws in ops._wgrad_ws.values():
        ws.fill_(0xFF)                    # every fp32 word 0xFFFFFFFF: a NaN
    assert bool(torch.isnan(next(iter(ops._wgrad_ws.values()))[:4].view(torch.float32)).all())


@pytest.mark.parametrize("c", R.W3_CASES + R.W4_CASES, ids=_id)
def test_wgrad_exact_case_equals_fp64(c, splits):
    """Integer operands: the fp32 result through any row ranges, partial tiles and the reduce is the fp64 value.  Also:
    the library's split count is the plan's, a second call gives equal bits, a call over a workspace full of NaNs is
    still exact (every partial tile the reduce reads was written), and no flag wait hit its bound."""
    splits(c.splits)
    plan = R.plan_of(c)
    assert _library_nsplit(c) == plan.nsplit, (c.name, _library_nsplit(c), plan)
    x, dy = (_dev(t) for t in R.wgrad_operands(c.name))
    want = R.expected_f32(R.wgrad_ref(c.name).dw)
    op = ops.conv3x3_wgrad if c.taps == 3 else ops.conv4x4_wgrad
    dw = op(x, dy)
    _assert_equal(dw, want, "conv_wgrad." + c.name)
    assert torch.equal(dw, op(x, dy)), "a second call gave other bits"
    _fill_workspaces_with_nans()
    _assert_equal(op(x, dy), want, "conv_wgrad." + c.name + ".nan_workspace")
    assert ops.N.lib().lss_conv2d_wgrad_timeouts() == 0, "a flag wait of the direct wgrad kernel hit its bound"


@pytest.mark.parametrize("c", [c for c in R.W3_CASES + R.W4_CASES if c.bound], ids=_id)
def test_wgrad_bound_case_against_fp64(c, splits, report):
    splits(c.splits)
    assert _library_nsplit(c) == R.plan_of(c).nsplit
    x, dy = (_dev(t) for t in R.wgrad_operands(c.name, False))
    ref = R.wgrad_ref(c.name, False)
    dw = (ops.conv3x3_wgrad if c.taps == 3 else ops.conv4x4_wgrad)(x, dy)
    tag = "conv_wgrad." + c.name
    assert dw.dtype == torch.float32
    _report(report, tag, *R.check(dw, ref.dw, ref.bound, tag), ref.bound, ref.dw)
    assert ops.N.lib().lss_conv2d_wgrad_timeouts() == 0


@pytest.mark.parametrize("shape", R.GEMM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_gemm_fallback_exact(shape, splits):
    """LSS_WGRAD_DIRECT=0: to_channel_major_kernel + the split-K linear_mfma_kernel + the reduce, on integer operands:
    exact too.  The last three shapes are ones only this path takes (W < 8, W > 224, channels no multiple of 64)."""
    B, H, W, Cin, Cout = shape
    size = lambda: ops.N.lib().lss_conv2d_wgrad_workspace_bytes(B, H, W, Cin, Cout)  # noqa: E731
    splits(None)
    plan, direct_size = R.wgrad_plan(B, H, W, Cin, Cout), size()
    assert (plan is None) == (shape in R.GEMM_ONLY)
    splits(None, direct="0")
    if plan is not None:   # with the switch on the shape is the direct kernel's: the fallback's workspace is another
        assert direct_size == plan.nsplit * 9 * Cout * Cin * 4 and size() != direct_size
    else:
        assert size() == direct_size
    name = "gemm_%dx%dx%d_c%d_%d" % shape
    x, dy = R.make_pair(name, (B, H, W, Cin), (B, H, W, Cout), True)
    ref = R.wgrad_case_reference(x, dy, 3, True)
    dw = ops.conv3x3_wgrad(_dev(x), _dev(dy))
    _assert_equal(dw, R.expected_f32(ref.dw), "conv_wgrad." + name)
    assert torch.equal(dw, ops.conv3x3_wgrad(_dev(x), _dev(dy)))


@pytest.mark.parametrize("c", R.S2_CASES, ids=_id)
def test_stride2_wgrad_over_phase_planes_exact(c, splits):
    """modules.conv_s2_wgrad_phase_planes (K9w on the space-to-depth input, then the tap / phase gather) on integers."""
    splits(None)
    R.plan_of(c)
    x, dy = (_dev(t) for t in R.s2_operands(c.name))
    want = R.expected_f32(R.s2_ref(c.name).dw)
    gw = M.conv_s2_wgrad_phase_planes(x, dy, c.K)
    _assert_equal(gw, want, "conv_wgrad." + c.name)
    assert torch.equal(gw, M.conv_s2_wgrad_phase_planes(x, dy, c.K))
    _fill_workspaces_with_nans()
    _assert_equal(M.conv_s2_wgrad_phase_planes(x, dy, c.K), want, "conv_wgrad." + c.name + ".nan_workspace")
    assert ops.N.lib().lss_conv2d_wgrad_timeouts() == 0


@pytest.mark.parametrize("c", [c for c in R.S2_CASES if c.bound], ids=_id)
def test_stride2_wgrad_bound_case_against_fp64(c, splits, report):
    splits(None)
    x, dy = (_dev(t) for t in R.s2_operands(c.name, False))
    ref = R.s2_ref(c.name, False)
    tag = "conv_wgrad." + c.name
    _report(report, tag, *R.check(M.conv_s2_wgrad_phase_planes(x, dy, c.K), ref.dw, ref.bound, tag), ref.bound, ref.dw)
    assert ops.N.lib().lss_conv2d_wgrad_timeouts() == 0


# ----------------------------------------------------------------------------------------------------------------------
# upsample + concat and its adjoint
# ----------------------------------------------------------------------------------------------------------------------
def _adjoint(g, c, rows, monkeypatch):
    """ops.upsample_bwd_nhwc with LSS_UPSAMPLE_BWD_ROWS on (the default) or off; returns (dx, the form it took)."""
    monkeypatch.delenv("LSS_UPSAMPLE_BWD_ROWS", raising=False)
    if not rows:
        monkeypatch.setenv("LSS_UPSAMPLE_BWD_ROWS", "0")
    dx = ops.upsample_bwd_nhwc(g, c.C2, c.Cx, c.up)
    monkeypatch.delenv("LSS_UPSAMPLE_BWD_ROWS", raising=False)
    return dx, R.adjoint_form(c.W, c.up, rows)


@pytest.mark.parametrize("c", [c for c in R.UP_CASES if c.exact], ids=_id)
def test_upsample_cat_and_adjoint_exact(c, monkeypatch):
    """up = 3 at dyadic ratios: both kernels' fp32 arithmetic is exact (asserted in the helper), so each output is the
    fp64 value rounded once to bf16; the sentinel of x2 passes through the concat and stays out of dx."""
    x, x2, g = R.up_operands(c.name)
    ref = R.up_ref(c.name)
    cat = ops.upsample_cat_nhwc(_dev(x), None if x2 is None else _dev(x2), c.up)
    _assert_equal(cat, R.expected_bf16(ref.cat), "conv_wgrad." + c.name + ".cat")
    if c.C2:
        assert bool((cat[..., :c.C2] == R.SENTINEL).all())
    want = R.expected_bf16(ref.dx)
    for rows in (True, False):
        dx, form = _adjoint(_dev(g), c, rows, monkeypatch)
        _assert_equal(dx, want, "conv_wgrad.%s.dx.%s" % (c.name, form))


@pytest.mark.parametrize("c", [c for c in R.UP_CASES if not c.exact], ids=_id)
def test_upsample_cat_and_adjoint_bound_case(c, monkeypatch, report):
    x, x2, g = R.up_operands(c.name)
    ref = R.up_ref(c.name)
    tag = "conv_wgrad." + c.name
    cat = ops.upsample_cat_nhwc(_dev(x), None if x2 is None else _dev(x2), c.up)
    assert cat.dtype == torch.bfloat16
    _report(report, tag + ".cat", *R.check(cat, ref.cat, ref.cat_bound, tag + ".cat"), ref.cat_bound, ref.cat)
    if c.C2:
        assert torch.equal(cat[..., :c.C2].cpu(), x2.bfloat16())
    forms = set()
    for rows in (True, False):
        dx, form = _adjoint(_dev(g), c, rows, monkeypatch)
        forms.add(form)
        assert dx.dtype == torch.bfloat16
        t = "%s.dx.%s" % (tag, form)
        _report(report, t, *R.check(dx, ref.dx, ref.dx_bound, t), ref.dx_bound, ref.dx)
    assert "walk" in forms


def test_upsample_cases_reach_all_three_adjoint_forms():
    assert {R.adjoint_form(c.W, c.up) for c in R.UP_CASES} == {"rows8", "rows12", "walk"}
