"""The helper of the weight-gradient / upsample-adjoint kernel tests (tests/conv_wgrad_ref.py) tested on the CPU: the
case tables reach the plan facts they state, every exact case meets its exactness precondition, the two derivations of
each reference agree, a correct float32 evaluation passes every bound, and every planted error is rejected by a
committed EXACT case (by inequality) and a committed BOUND case (through `check`) and raises NotExercised where a case
cannot show it."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import conv_wgrad_ref as R

STRIDE1 = R.W3_CASES + R.W4_CASES
_id = lambda c: c.name  # noqa: E731


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ----------------------------------------------------------------------------------------------------------------------
# plan and case tables
# ----------------------------------------------------------------------------------------------------------------------
def test_plan_constants_and_slot_counts():
    assert [R.wgrad_plan(1, 4, 32 * kb, 64, 64).nxs for kb in range(1, 8)] == [8, 8, 8, 7, 5, 4, 4]
    assert R.wgrad_plan(1, 4, 225, 64, 64) is None and R.wgrad_plan(1, 4, 7, 64, 64) is None
    assert R.wgrad_plan(1, 4, 16, 72, 64) is None and R.wgrad_plan(1, 4, 16, 64, 40) is None
    p = R.wgrad_plan(4, 100, 100, 64, 64)   # layer1 at the bench batch: 408 padded rows over 256 -> 204 splits of 2 -> 3
    assert (p.KB, p.nxs, p.rows_total, p.rows_per, p.nsplit) == (4, 7, 408, 3, 136)


def test_plan_reads_the_splits_override(monkeypatch):
    monkeypatch.delenv("LSS_WGRAD_SPLITS", raising=False)
    assert R.wgrad_plan(5, 3, 33, 128, 64).nsplit == 9
    monkeypatch.setenv("LSS_WGRAD_SPLITS", "1")
    assert R.wgrad_plan(5, 3, 33, 128, 64).nsplit == 1
    monkeypatch.setenv("LSS_WGRAD_SPLITS", "0")       # the library raises anything below 1 to 1
    assert R.wgrad_plan(5, 3, 33, 128, 64).nsplit == 1
    assert R.wgrad_plan(5, 3, 33, 128, 64, splits=2).rows_per == 13


@pytest.mark.parametrize("c", STRIDE1 + R.S2_CASES, ids=_id)
def test_case_reaches_the_plan_facts_it_states(c, monkeypatch):
    monkeypatch.delenv("LSS_WGRAD_SPLITS", raising=False)
    assert c.facts
    R.plan_of(c)


@pytest.mark.parametrize("c", STRIDE1, ids=_id)
def test_plan_is_the_librarys_host_plan(c, monkeypatch):
    """lss_conv2d_wgrad_workspace_bytes is host code: the library's split count equals the Python plan's without a GPU
    (the GPU test repeats it where the kernels run); with LSS_WGRAD_DIRECT=0 the workspace is the fallback's."""
    from lss2_multimodal_nu_amd import _native as N
    from lss2_multimodal_nu_amd import build_native
    build_native.build(verbose=False)
    monkeypatch.delenv("LSS_WGRAD_DIRECT", raising=False)
    monkeypatch.delenv("LSS_WGRAD_SPLITS", raising=False)
    if c.splits is not None:
        monkeypatch.setenv("LSS_WGRAD_SPLITS", str(c.splits))
    fn = N.lib().lss_conv2d_wgrad_workspace_bytes if c.taps == 3 else N.lib().lss_conv2d_wgrad4x4_workspace_bytes
    per = c.taps * c.taps * c.Cout * c.Cin * 4
    nbytes = fn(c.B, c.H, c.W, c.Cin, c.Cout)
    assert nbytes == R.plan_of(c).nsplit * per
    monkeypatch.setenv("LSS_WGRAD_DIRECT", "0")
    assert fn(c.B, c.H, c.W, c.Cin, c.Cout) != nbytes


def test_case_tables_are_the_issues():
    shapes = lambda cs: [(c.B, c.H, c.W, c.Cin, c.Cout, c.splits) for c in cs]  # noqa: E731
    assert shapes(R.W3_CASES) == [(1, 1, 8, 64, 64, None), (3, 2, 9, 64, 128, None), (5, 3, 33, 128, 64, 1),
                                  (4, 7, 129, 64, 64, 1), (3, 6, 161, 64, 64, 2), (2, 5, 224, 64, 192, 1),
                                  (2, 9, 100, 192, 128, None), (1, 46, 40, 64, 64, None), (2, 30, 40, 64, 64, None),
                                  (1, 40, 97, 64, 64, None)]
    assert shapes(R.W4_CASES) == [(1, 1, 8, 64, 64, None), (3, 2, 9, 64, 64, None), (4, 5, 129, 64, 128, 1),
                                  (2, 3, 224, 128, 64, 1), (2, 30, 40, 64, 64, None)]
    assert [(c.K, c.B, c.H, c.W, c.C, c.Co) for c in R.S2_CASES] == [
        (3, 2, 6, 18, 16, 64), (1, 3, 4, 16, 32, 128), (7, 2, 6, 22, 16, 64), (7, 1, 2, 16, 64, 128), (3, 1, 10, 66, 16, 64)]
    # the bound runs the issue names are among the bound cases, and every bound case keeps B H W <= 2000
    assert {1, 2} <= {i for i, c in enumerate(R.W3_CASES) if c.bound} and R.W4_CASES[1].bound
    assert R.S2_CASES[0].bound and R.S2_CASES[2].bound
    assert all(c.B * c.H * c.W <= 2000 for c in STRIDE1 + R.S2_CASES if c.bound)
    assert [R.wgrad_plan(*s) for s in R.GEMM_ONLY] == [None] * 3
    assert all(R.wgrad_plan(*s) is not None for s in R.GEMM_CASES[:3])
    assert [(c.B, c.H, c.W, c.Cx, c.C2, c.up) for c in R.UP_CASES] == [
        (2, 3, 3, 8, 0, 3), (1, 3, 11, 64, 8, 3), (2, 11, 11, 16, 64, 3), (1, 11, 43, 8, 0, 3),
        (2, 2, 2, 8, 0, 2), (1, 7, 9, 64, 64, 2), (1, 100, 100, 8, 0, 2), (2, 25, 25, 16, 8, 4), (1, 2, 5, 8, 8, 4)]
    assert [c.exact for c in R.UP_CASES] == [True] * 4 + [False] * 5


# ----------------------------------------------------------------------------------------------------------------------
# the weight gradient's references
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", STRIDE1, ids=_id)
def test_stride1_exact_case_precondition_and_the_two_derivations(c):
    x, dy = R.wgrad_operands(c.name)
    R.assert_exact_precondition(x, dy)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy)
    ref = R.wgrad_ref(c.name)            # asserts 6 B H W < 2^24 and S <= 6 B H W
    assert torch.equal(ref.dw, R.wgrad_reference(x, dy, c.taps))       # integers: the two derivations agree exactly
    assert float(ref.bound.max()) == 0.0
    R.expected_f32(ref.dw)
    if c.H == 1:                         # every tap that needs another row is an exact zero
        live = R.DISP[c.taps].index(0)
        dead = [t for t in range(c.taps) if t != live]
        assert float(ref.dw[:, :, dead].abs().max()) == 0.0 and float(ref.dw[:, :, live].abs().max()) > 0
    # torch's own fp32 evaluation (one possible order) gives the same bits
    f32 = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), tuple(ref.dw.shape), dy.permute(0, 3, 1, 2), padding=1) \
        if c.taps == 3 else None
    assert f32 is None or torch.equal(f32.double(), ref.dw)


@pytest.mark.parametrize("c", [c for c in STRIDE1 if c.bound], ids=_id)
def test_stride1_bound_case_derivations_agree_and_fp32_passes(c):
    x, dy = R.wgrad_operands(c.name, False)
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(dy.bfloat16().float(), dy)
    ref = R.wgrad_ref(c.name, False)
    assert _rel(ref.dw, R.wgrad_reference(x, dy, c.taps)) <= 1e-12
    xn = x.permute(0, 3, 1, 2) if c.taps == 3 else F.pad(x.permute(0, 3, 1, 2), (2, 1, 2, 1))
    f32 = torch.nn.grad.conv2d_weight(xn, tuple(ref.dw.shape), dy.permute(0, 3, 1, 2), padding=1 if c.taps == 3 else 0)
    R.check(f32, ref.dw, ref.bound, c.name)
    # the bound sees one product: at B H W <= 2000 it stays below a quarter of the typical |dy x| = 2 / pi = 0.64
    assert float(ref.bound.max()) < 0.16


@pytest.mark.parametrize("c", R.S2_CASES, ids=_id)
def test_stride2_references(c):
    x, dy = R.s2_operands(c.name)
    ref = R.s2_ref(c.name)
    assert torch.equal(ref.dw, R.s2_wgrad_reference(x, dy, c.K))
    R.expected_f32(ref.dw)
    if c.H == 2:   # one phase-plane row: kernel rows that need another output row are exact zeros
        assert float(ref.n.min()) == 0.0 and float(ref.dw[:, :, ref.n == 0].abs().max()) == 0.0
    if c.bound:
        xb, dyb = R.s2_operands(c.name, False)
        rb = R.s2_ref(c.name, False)
        assert _rel(rb.dw, R.s2_wgrad_reference(xb, dyb, c.K)) <= 1e-12
        f32 = torch.nn.grad.conv2d_weight(xb.permute(0, 3, 1, 2), tuple(rb.dw.shape), dyb.permute(0, 3, 1, 2), stride=2,
                                          padding=c.K // 2)
        R.check(f32, rb.dw, rb.bound, c.name)


# ----------------------------------------------------------------------------------------------------------------------
# upsample + concat and its adjoint
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.UP_CASES, ids=_id)
def test_upsample_reference_is_torchs(c):
    x, x2, g = R.up_operands(c.name)
    ref = R.up_ref(c.name)               # an exact case: asserts that the kernels' fp32 formulas are exact
    xf = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    upx = F.interpolate(xf, scale_factor=c.up, mode="bilinear", align_corners=True)
    want = upx if x2 is None else torch.cat([x2.double().permute(0, 3, 1, 2), upx], 1)
    assert _rel(ref.cat, want.detach().permute(0, 2, 3, 1)) <= 1e-12
    upx.backward(g.double()[..., c.C2:].permute(0, 3, 1, 2))
    assert _rel(ref.dx, xf.grad.permute(0, 2, 3, 1)) <= 1e-12
    if c.exact:
        assert ref.cat_bound is None
        if c.C2:
            assert float(ref.cat[..., :c.C2].min()) == R.SENTINEL == float(ref.cat[..., :c.C2].max())
        assert float(ref.dx.abs().max()) < R.SENTINEL / 2      # no sentinel in dx
    else:
        # the kernels' formulas in float32, rounded to bf16, lie inside the derived bounds
        cat32 = R.cat_f32(x, c.up).bfloat16().float()
        cat32 = cat32 if x2 is None else torch.cat([x2, cat32], 3)
        R.check(cat32, ref.cat, ref.cat_bound, c.name + ".cat")
        R.check(R.adjoint_f32(g, c.C2, c.Cx, c.up).bfloat16().float(), ref.dx, ref.dx_bound, c.name + ".dx")
        # and the bounds are those of one bf16 rounding, not of a wrong weight
        assert float((ref.dx_bound / ref.dx.abs().clamp_min(1.0)).max()) < 2.0 ** -7


def test_upsample_cases_reach_all_three_adjoint_forms():
    forms = {R.adjoint_form(c.W, c.up) for c in R.UP_CASES}
    assert forms == {"rows8", "rows12", "walk"}
    assert {R.adjoint_form(c.W, c.up) for c in R.UP_CASES if c.exact} == {"rows12"}
    assert {R.adjoint_form(c.W, c.up, False) for c in R.UP_CASES} == {"walk"}
    assert R.adjoint_form(100, 2) == "rows8" and R.adjoint_form(25, 4) == "rows12" and R.adjoint_form(5, 4) == "walk"


def test_dyadic_ratios_are_exact_in_float32():
    for n, r in ((3, 0.25), (11, 5.0 / 16), (43, 21.0 / 64)):
        r32, i0, _, l = R._axis_f32(n, 3)
        assert float(r32) == r
        s = r * np.arange(3 * n)
        assert np.array_equal(i0, np.floor(s).astype(np.int64)) and np.array_equal(l.astype(np.float64), s - np.floor(s))
        assert np.array_equal(l * 64, np.round(l * 64))


# ----------------------------------------------------------------------------------------------------------------------
# planted errors
# ----------------------------------------------------------------------------------------------------------------------
W3 = [c.name for c in R.W3_CASES]
W4 = [c.name for c in R.W4_CASES]
S2 = [c.name for c in R.S2_CASES]
UP = [c.name for c in R.UP_CASES]
# plant -> (family, the EXACT case that rejects it, the BOUND case that rejects it)
REJECTED_BY = {
    "one_position_dropped": ("w", W3[1], W3[1]),
    "row_wrap": ("w", W3[1], W3[2]),
    "image_boundary_leak": ("w", W3[2], W3[2]),
    "last_column_dropped": ("w", W3[3], W3[1]),
    "last_k_block_dropped": ("w", W3[2], W3[2]),       # KB = 2: one live position is all it drops
    "ky_kx_swapped": ("w", W3[0], W3[1]),
    "channel_tiles_swapped": ("w", W3[6], W3[6]),
    "last_split_dropped": ("w", W3[7], W3[1]),
    "taps4x4_shifted": ("w", W4[1], W4[1]),
    "tap_rows_swapped": ("w", W4[0], W4[1]),
    "phase_swapped": ("s2", S2[0], S2[2]),
    "k1_wrong_phase": ("s2", S2[1], S2[1]),
    "adjoint_not_align_corners": ("up", UP[0], UP[4]),
    "adjoint_last_row_clamp": ("up", UP[2], UP[5]),
    "adjoint_window_one_short": ("up", UP[3], UP[8]),
    "c_off_ignored": ("up", UP[2], UP[5]),
}


def test_every_plant_has_its_cases():
    assert set(REJECTED_BY) == set(R.PLANTS) and len(R.PLANTS) == 16


def _planted(family, name, plant, exact):
    """(planted, unplanted reference, bound) of a committed case."""
    if family == "w":
        ref = R.wgrad_ref(name, exact)
        return R.wgrad_planted(name, plant, exact).dw, ref.dw, ref.bound
    if family == "s2":
        ref = R.s2_ref(name, exact)
        return R.s2_case_reference(*R.s2_operands(name, exact), R.S2_BY_NAME[name].K, exact, plant).dw, ref.dw, ref.bound
    c = R.UP_BY_NAME[name]
    assert c.exact == exact
    ref = R.up_ref(name)
    return R.up_reference(*R.up_operands(name), c.up, c.exact, plant).dx, ref.dx, ref.dx_bound


@pytest.mark.parametrize("plant", R.PLANTS)
def test_an_exact_case_rejects_the_plant(plant):
    family, name, _ = REJECTED_BY[plant]
    planted, ref, _ = _planted(family, name, plant, True)
    if family == "up":
        assert not torch.equal(R.expected_bf16(planted), R.expected_bf16(ref))
    else:
        assert not torch.equal(planted.float(), R.expected_f32(ref))


@pytest.mark.parametrize("plant", R.PLANTS)
def test_a_bound_case_rejects_the_plant_through_check(plant):
    family, _, name = REJECTED_BY[plant]
    planted, ref, bound = _planted(family, name, plant, False)
    got = planted.float().bfloat16().float() if family == "up" else planted.float()   # as a kernel would return it
    with pytest.raises(AssertionError, match="outside the derived bound"):
        R.check(got, ref, bound, plant)


def _big_bound_pair():
    g = torch.Generator().manual_seed(5)
    return (R.bf16_round(torch.randn(16, 100, 100, 8, generator=g)), R.bf16_round(torch.randn(16, 100, 100, 8, generator=g)))


@pytest.mark.parametrize("plant", R.PLANTS)
def test_a_case_that_cannot_show_the_plant_raises_not_exercised(plant):
    family = REJECTED_BY[plant][0]
    with pytest.raises(R.NotExercised):
        if plant in ("one_position_dropped", "last_column_dropped", "last_k_block_dropped"):
            # 160 000 positions: (n + 2) u S is about a thousand products wide - why bound cases keep B H W <= 2000
            R.wgrad_case_reference(*_big_bound_pair(), 3, False, R.wgrad_plan(16, 100, 100, 64, 64), plant)
        elif plant in ("row_wrap", "image_boundary_leak"):
            R.wgrad_planted(W3[0], plant)                       # one row, one image
        elif plant == "ky_kx_swapped":                          # constant operands on a square image: dw is symmetric
            R.wgrad_case_reference(torch.ones(1, 5, 5, 8), torch.ones(1, 5, 5, 8), 3, True, None, plant)
        elif plant == "channel_tiles_swapped":
            R.wgrad_planted(W3[1], plant)                       # one Cin tile
        elif plant == "last_split_dropped":
            R.wgrad_planted(W3[6], plant)                       # the last split holds a pad row only
        elif plant in R.W4_PLANTS:
            R.wgrad_planted(W3[1], plant)                       # not the 4x4 form
        elif plant == "phase_swapped":
            R.s2_case_reference(*R.s2_operands(S2[1]), 1, True, plant)
        elif plant == "k1_wrong_phase":
            R.s2_case_reference(*R.s2_operands(S2[0]), 3, True, plant)
        elif plant == "adjoint_not_align_corners":
            x, _, _ = R.up_operands(UP[4])
            R.up_reference(x, None, x, 1, False, plant)         # up = 1
        elif plant == "c_off_ignored":
            R.up_reference(*R.up_operands(UP[0]), 3, True, plant)   # no skip tensor
        else:   # the last high-res rows and columns carry no gradient: nothing for the bottom / right edge to lose
            x, x2, g = R.up_operands(UP[2])
            g = g.clone()
            g[:, -5:, :, 64:] = 0
            g[:, :, -5:, 64:] = 0
            R.up_reference(x, x2, g, 3, True, plant)
    # and a plant of another family is never exercised
    with pytest.raises(R.NotExercised):
        if family == "up":
            R.wgrad_planted(W3[1], plant)
        else:
            R.up_reference(*R.up_operands(UP[0]), 3, True, plant)
