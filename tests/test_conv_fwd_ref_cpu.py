"""tests/conv_fwd_ref.py on the CPU: the case table reaches the instantiations it names, the exact cases are provably
exact, the ambiguity cap holds, the fp64 reference agrees with a second derivation, a float32 emulation of the correct
arithmetic lies inside every bound, and every planted error is rejected."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_fwd_ref as R

_id = lambda c: c.name  # noqa: E731


def test_case_table_reaches_what_it_names():
    """make_inputs asserts expected_inst(c) == c.inst; here: the table covers every reachable instantiation once."""
    for c in R.CASES:
        assert R.expected_inst(c) == c.inst, c.name
    exact = {c.inst for c in R.EXACT_CASES}
    for inst in ("ring<0,0,8,0>", "ring<0,1,8,0>", "ring<1,0,7,0>", "ring<1,1,7,0>", "ring<1,0,7,1>", "ring<1,1,7,1>",
                 "direct<bf16,plain>", "direct<bf16,fused>", "direct<f32,plain>", "direct<f32,fused>",
                 "lds<2,64,0,3,64,1,1,1>", "lds<2,128,0,3,64,1,1,1>", "lds<2,128,1,3,32,1,1,1>+src", "lds<2,128,1,3,64,1,1,1>",
                 "lds<1,64,0,3,64,1,0,1>", "lds<2,64,0,3,64,1,0,1>", "lds<1,128,0,3,64,1,0,1>", "lds<2,128,0,3,64,1,0,1>",
                 "lds<1,128,0,3,64,2,0,1>", "lds<2,128,0,3,32,1,0,1>", "lds<1,64,0,2,64,1,0,1>", "lds<1,128,0,4,64,1,0,1>",
                 "lds<2,128,1,3,32,1,0,1>+src", "lds<2,128,1,3,32,1,0,1>", "lds<2,128,1,3,64,1,0,1>", "lds<1,128,1,3,64,1,0,1>",
                 "lds<1,128,2,1,64,1,0,1>", "lds<1,64,2,2,64,1,0,1>", "lds<1,128,2,2,64,2,0,1>", "lds<2,128,2,2,64,1,0,1>",
                 "lds<1,64,2,4,64,1,0,2>", "lds<2,64,2,4,64,1,0,1>"):
        assert inst in exact, inst
    assert "lds<1,64,2,4,64,1,0,1>" not in {c.inst for c in R.CASES}   # the one-tap stem form: not built
    # the image sizes of the tile cases are no multiples of the 16-wide, 8- or 16-high tiles
    for c in R.CASES:
        Ho, Wo = R.out_hw(c)
        if c.kernel == "tile" and c.name != "h_c128_n4" and c.name != "b_h_c128_n4":
            assert Wo % 16 and Ho % 8, c.name
        assert c.B <= 8 and c.H * c.up <= 37 or c.kernel == "ring", c.name
    assert any(c.Cout % 64 for c in R.EXACT_CASES if c.kernel == "tile")
    for env, inst in (({"LSS_CONV_DIRECT": "1"}, "direct<bf16,plain>"), ({"LSS_CONV_RT": "2", "LSS_CONV_KC": "32"},
                                                                         "lds<2,128,0,3,32,1,0,1>")):
        assert R.tile_inst(R.BY_NAME["t0_wide_rt2_res"], env) == inst


@pytest.mark.parametrize("c", R.EXACT_CASES, ids=_id)
def test_exact_cases_are_exact_in_fp32(c):
    """ref_conv runs _assert_exact (sum |x| |w| / g < 2^24, operands on the grid) and, for the fused cases, compares the
    float32 emulation of the kernels' blend with the fp64 blend bit for bit; the float32 emulation of the whole chain
    then has to reproduce the rounded reference exactly, in torch's own summation order."""
    ins, ref = R.make_inputs(c.name), R.reference(c.name)
    assert float(ref.bound.max()) == 0.0 and ref.share == 0.0
    for t in (ins["x"], ins["x2"], ins["residual"]):
        assert t is None or float(t.abs().max()) <= 3.0
    assert float(ins["w"].abs().max()) <= 2.0 and bool((ins["w"] == ins["w"].round()).all())
    want = R.expected(c, ref.out)
    got, got2, _ = R.emulate_f32(c, ins)
    assert got.dtype == want.dtype and torch.equal(got, want)
    if c.entry == "dual":
        assert torch.equal(got2, R.expected(c, ref.out2))
        assert bool((ref.out2 < 0).any()) and bool((ref.out >= 0).all())   # a ReLU on the second output would show


def test_constant_map_blends_to_itself_in_float32():
    """Construction (b): the four-weight form of conv_ring.hip:102 in float32 returns c to within a few ulp for every
    upsampling factor and size, so its bf16 rounding is c."""
    g = torch.Generator().manual_seed(5)
    for up in (2, 3, 4):
        for H, W in ((5, 7), (9, 13), (16, 80), (13, 65), (7, 33)):
            x = torch.randint(-3, 4, (2, 1, 1, 8), generator=g).float().expand(2, H, W, 8).contiguous()
            v = R.blend_f32(x, up)
            want = x[:, :1, :1].expand_as(v)
            assert float((v - want).abs().max()) <= 8 * 3 * R.U32
            assert torch.equal(v.bfloat16().float(), want)


def test_dyadic_ratios_blend_exactly():
    """Construction (a): torch's fp32 and fp64 interpolation, the fp64 gather and the float32 emulation of the kernels'
    blend agree bit for bit at up = 3, H, W in {3, 11, 43}."""
    g = torch.Generator().manual_seed(6)
    for H, W in ((3, 11), (11, 11), (11, 43), (43, 3)):
        x = torch.randint(-3, 4, (1, H, W, 4), generator=g).double()
        v = R.blend64(x, 3)[0]
        for dt in (torch.float32, torch.float64):
            t = F.interpolate(x.to(dt).permute(0, 3, 1, 2), scale_factor=3, mode="bilinear", align_corners=True)
            assert torch.equal(t.permute(0, 2, 3, 1).double(), v)
        assert torch.equal(R.blend_f32(x.float(), 3).double(), v)


@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_reference_agrees_with_a_second_derivation(c):
    """The hand-written gather + F.conv2d with the re-derived pack layouts against F.interpolate + im2col (and, for the
    two data-gradient packs, autograd of the forward conv)."""
    ins = R.make_inputs(c.name)
    if c.up > 1 and c.kind == "bound" and c.dt == R.BF16:
        # the reference rounds the blended operand: compare the blend itself
        v = R.blend64(ins["x"].double(), c.up)[0]
        t = F.interpolate(ins["x"].double().permute(0, 3, 1, 2), scale_factor=c.up, mode="bilinear", align_corners=True)
        assert float((t.permute(0, 2, 3, 1) - v).abs().max()) <= 1e-12 * float(v.abs().max())
        return
    raw, second = R.reference(c.name).raw, R.ref_conv_second(c, ins)
    if c.wpack == "s2_dgrad":
        raw = raw[:, :, 1:1 + c.H, 1:1 + c.W]
    assert raw.shape == second.shape
    assert float((raw - second).abs().max()) <= 1e-12 * float(raw.abs().max())


@pytest.mark.parametrize("c", R.BOUND_CASES, ids=_id)
def test_float32_emulation_lies_inside_the_bound(c):
    ins, ref = R.make_inputs(c.name), R.reference(c.name)
    assert ref.share <= R.AMBIGUOUS_CAP, (c.name, ref.share)
    assert ref.share == 0.0 or (c.up > 1 and c.dt == R.BF16)   # only a blended bf16 operand can round either way
    got, got2, stats = R.emulate_f32(c, ins)
    e = R.check(got, ref.out, ref.bound, c.name)
    assert e[0] > 0.0
    if got2 is not None:
        R.check(got2, ref.out2, ref.bound2, c.name + ".y2")
    if c.stats:
        R.check(stats, ref.stats, ref.stats_bound, c.name + ".stats")
    # the bound is no blank cheque: a bf16 output's stays below one ulp of the largest output (half an ulp of rounding,
    # the rest the ambiguous operands), a head's below 2^-5 of the largest logit (its inputs' ambiguous operands)
    scale = float(ref.out.abs().max())
    assert float(ref.bound.max()) <= (2.0 ** -7 if not c.head_n else 2.0 ** -5) * scale, c.name


def test_ambiguity_cap_and_what_randn_would_give():
    shares = {c.name: R.reference(c.name).share for c in R.BOUND_CASES if c.up > 1 and c.dt == R.BF16}
    assert len(shares) >= 6 and all(0.0 < s <= R.AMBIGUOUS_CAP for s in shares.values()), shares
    c = R.BY_NAME["b_t1_kc32_src_up2"]
    ins = dict(R.make_inputs(c.name))
    ins["x"] = torch.randn(ins["x"].shape, generator=torch.Generator().manual_seed(1)).bfloat16()
    assert R.ref_conv(c, ins).share > R.AMBIGUOUS_CAP   # plain randn x1: the reason for the offset inputs


def test_blend_delta_covers_the_kernels_fractions():
    """The kernels' 16-bit fractions (float32 coordinates, rounding, clamp) against the exact rational fractions: the
    difference of the source COORDINATE i0 + frac is inside blend_delta for every size the cases use and more."""
    for n_in in (2, 3, 5, 7, 9, 11, 13, 16, 33, 43, 65, 80, 100, 200):
        for up in (2, 3, 4):
            i0, _, f = R._axis64(n_in, n_in * up)
            j0, _, q = R._axis32(n_in, n_in * up)
            d = np.abs((i0 + f) - (j0 + q.astype(np.float64)))
            assert float(d.max()) <= R.blend_delta(n_in), (n_in, up, float(d.max()))


def _first_rejection(plant, cases, exact):
    for c in cases:
        ins, ref = R.make_inputs(c.name), R.reference(c.name)
        try:
            bad = R.ref_conv(c, ins, plant=plant)
        except R.NotExercised:
            continue
        pairs = [(bad.out, ref.out, ref.bound)] + ([(bad.out2, ref.out2, ref.bound2)] if c.entry == "dual" else [])
        if exact:
            if any(not torch.equal(R.expected(c, b, strict=False), R.expected(c, r)) for b, r, _ in pairs):
                return c.name
            continue
        for b, r, bound in pairs:
            wrong = R.bf16_rn(b) if not (c.head_n or c.dt == R.F32) else b   # what a kernel with this error would store
            try:
                R.check(wrong, r, bound, c.name)
            except AssertionError:
                return c.name
    return None


@pytest.mark.parametrize("plant", R.PLANTS)
def test_every_plant_is_rejected(plant):
    """`check` rejects the planted error on a committed bound case, and an exact case rejects it by inequality."""
    small = lambda cs: sorted(cs, key=lambda c: c.B * c.H * c.W * c.up * c.up * (c.Cx + c.C2) * c.Cout)  # noqa: E731
    assert _first_rejection(plant, small(R.BOUND_CASES), False) is not None, plant
    if plant != "shift_before_scale":   # the exact cases carry no scale or shift
        assert _first_rejection(plant, small(R.EXACT_CASES), True) is not None, plant


def test_not_exercised_is_raised_where_a_case_cannot_show_a_plant():
    c = R.BY_NAME["t0_narrow_rt1"]
    for plant in ("align_corners_false", "concat_halves_swapped", "residual_after_activation", "relu_on_second_output",
                  "phases_01_10_swapped", "head_bias_of_class_0", "shift_before_scale"):
        with pytest.raises(R.NotExercised):
            R.ref_conv(c, R.make_inputs(c.name), plant=plant)
    with pytest.raises(ValueError):
        R.ref_conv(c, R.make_inputs(c.name), plant="no_such_plant")
