"""tests/deform_attn_ref.py on its own, without a GPU: the reference is the F.grid_sample composition and the oracle's
explicit bilinear gather in float64, its three ways in agree, a float32 emulation of deform_attn_kernel (with and without
the contracted px statement) sits inside every derived bound, no case is vacuous, and every planted error is rejected."""
import functools

import pytest
import torch

import deform_attn_ref as R
from oracle import vovnet_oracle as vo

_id = lambda c: c.name  # noqa: E731
V = R.VARIANT_BY_NAME
SEL_VARIANTS = [v for v in R.VARIANTS if not v.bias and not v.pts]


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@functools.lru_cache(maxsize=None)
def _case(name, kind, vname):
    c, v = R.BY_NAME[name], V[vname]
    ins = R.make_inputs(c, kind, v)
    return c, ins, R.ref_deform_attn(c, ins)


def _points(c, ins):
    pts = ins["ref_pts"] if ins["ref_pts"] is not None else R.grid_points(ins["ref_x"], ins["ref_y"])
    return pts.double().expand(c.B, c.H * c.W, 2)


def _full(c, ins):
    ol = ins["ol"].double().reshape(c.B, c.H * c.W, 192)
    return ol if ins["token_bias"] is None else ol + ins["token_bias"].double()[None]


def _close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# the reference is the operation
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_reference_is_grid_sample_and_the_oracle_gather(c):
    B, H, W = c.B, c.H, c.W
    N = H * W
    for kind in R.KINDS:
        for vname in ("nhwc_f32", "hm_bf16_bias", "pts_shared", "pts_per_sample"):
            _, ins, ref = _case(c.name, kind, vname)
            assert (ref.out.dtype, ref.bound.dtype) == (torch.float64, torch.float64)
            assert ref.out.shape == ref.bound.shape == ((B, N, 256) if V[vname].pts else (B, H, W, 256))
            assert bool((ref.bound > 0).all()) and bool(torch.isfinite(ref.bound).all())
            val, full, pts = ins["value"].double().reshape(B, N, 256), _full(c, ins), _points(c, ins)
            got = ref.out.reshape(B, N, 256)
            assert _close(got, R.grid_sample_composition(val, full, pts, H, W)), (kind, vname)
            off = full[..., :128].reshape(B, N, 8, 8, 2)
            aw = torch.softmax(full[..., 128:].reshape(B, N, 8, 8), -1)
            loc = (pts[:, :, None, None, :] + off / H).clamp(0, 1)
            want = torch.zeros(B, N, 8, 32, dtype=torch.float64)
            v = val.reshape(B, H, W, 8, 32)
            for h in range(8):
                gg = loc[:, :, h] * 2.0 - 1.0
                px, py = ((gg[..., 0] + 1) * W - 1) / 2, ((gg[..., 1] + 1) * H - 1) / 2
                s = vo.bilinear_zero_pad(v[:, :, :, h], px.reshape(B, -1), py.reshape(B, -1)).view(B, N, 8, 32)
                want[:, :, h] = (s * aw[:, :, h, :, None]).sum(2)
            assert _close(got, want.reshape(B, N, 256)), (kind, vname)


@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_three_ways_in_give_the_same_reference(c):
    for kind in R.KINDS:
        _, gi, grid = _case(c.name, kind, "nhwc_f32")
        _, _, pts = _case(c.name, kind, "pts_shared")
        assert torch.equal(pts.out.reshape(grid.out.shape), grid.out)
        _, bi, bias = _case(c.name, kind, "nhwc_f32_bias")
        assert torch.equal(bi["ol_full"], gi["ol"]) and torch.equal(bi["value"], gi["value"])
        # the split done in float64: the same problem to the last bits
        split = dict(bi, ol=bi["ol_full"].double() - bi["token_bias"].double().view(1, c.H, c.W, 192))
        assert _close(R.ref_deform_attn(c, split).out, grid.out)
        # the split as the model does it (one fp32 rounding): inside the bound that is told of that rounding
        cross = R.ref_deform_attn(c, bi, input_err=R.U32 * bi["ol"].abs())
        R.check(grid.out, bias.out, cross.bound, "%s.%s" % (c.name, kind))
        assert bool((cross.bound >= bias.bound).all())
        # layouts share the reference; bf16 values are their own problem
        assert torch.equal(_case(c.name, kind, "hm_f32")[2].out, grid.out)
        assert not torch.equal(_case(c.name, kind, "nhwc_bf16")[2].out, grid.out)


# ----------------------------------------------------------------------------------------------------------------------
# a float32 emulation of the kernel stays inside the bound
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_float32_emulation_is_inside_the_bound(c, kind):
    differ = 0
    for v in R.VARIANTS:
        _, ins, ref = _case(c.name, kind, v.name)
        outs = [R.emulate_f32(c, ins, contract) for contract in (False, True)]
        for contract, out in zip((False, True), outs):
            tag = "%s.%s.%s.%s" % (c.name, kind, v.name, "fma" if contract else "mul_add")
            assert out.dtype == (torch.bfloat16 if v.bf16 else torch.float32)
            R.check(out, ref.out, ref.bound, tag)
            ratio = float(((out.double() - ref.out).abs() / ref.bound).max())
            print("emulation %s error/bound %.4f bound/max %.3e position share %.2f"
                  % (tag, ratio, float(ref.bound.max() / ref.out.abs().max()), ref.pos_share))
        differ += int(not torch.equal(outs[0], outs[1]))
    if kind == "random" and c.name not in ("one_token", "full_blocks"):   # (a power-of-two size multiplies exactly)
        assert differ        # the two versions are two computations


def test_selector_emulation_is_exact():
    c = R.BY_NAME["full_blocks"]
    for v in SEL_VARIANTS:
        ins = R.make_inputs(c, "selector", v)
        want = R.selector_rows(c, ins)
        for contract in (False, True):
            assert torch.equal(R.emulate_f32(c, ins, contract), want)
        ref = R.ref_deform_attn(c, ins)
        assert torch.equal(ref.out.to(want.dtype), want) and torch.equal(ref.out, want.double())


# ----------------------------------------------------------------------------------------------------------------------
# no case is vacuous
# ----------------------------------------------------------------------------------------------------------------------
def test_case_table():
    assert [(c.name, c.B, c.H, c.W) for c in R.CASES] == [
        ("one_token", 1, 1, 1), ("odd_9", 1, 3, 3), ("odd_105_wide", 3, 5, 7), ("tall", 2, 14, 9), ("wide", 2, 9, 14),
        ("full_blocks", 2, 4, 8), ("very_wide", 1, 2, 33)]
    rows = {c.name: c.B * c.H * c.W for c in R.CASES}
    assert rows == dict(one_token=1, odd_9=9, odd_105_wide=105, tall=252, wide=252, full_blocks=64, very_wide=66)
    assert rows["odd_105_wide"] % 8 == 1 and rows["odd_9"] % 8 == 1 and rows["full_blocks"] % 8 == 0 and rows["tall"] % 8
    assert len(R.VARIANTS) == 10 and {(v.layout, v.bf16, v.bias) for v in R.VARIANTS if not v.pts} == {
        (lay, bf, bias) for lay in ("nhwc", "hm") for bf in (False, True) for bias in (False, True)}


@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_case_conditions(c):
    H, W = c.H, c.W
    for kind in ("random", "far"):
        for vname in ("nhwc_f32", "pts_per_sample"):
            _, ins, ref = _case(c.name, kind, vname)
            px, py = ref.px, ref.py
            # footprints that leave the image on each side, and (where the image has one) interior footprints
            assert bool((px < 0).any()) and bool((px > W - 1).any()) and bool((py < 0).any()) and bool((py > H - 1).any())
            if W > 1 and H > 1:
                assert bool(((px > 0) & (px < W - 1) & (py > 0) & (py < H - 1)).any()), (kind, vname)
            clamped = (ref.raw_x < 0) | (ref.raw_x > 1) | (ref.raw_y < 0) | (ref.raw_y > 1)
            share = float(clamped.double().mean())
            print("%s %s %s clamped share %.3f" % (c.name, kind, vname, share))
            if kind == "far":
                assert share >= 0.5
                assert bool(((ref.dpx == 0) & (ref.raw_x < 0)).any()) and bool(((ref.dpx == 0) & (ref.raw_x > 1)).any())
            else:
                assert share > 0.0 and (share < 1.0 or c.name == "one_token")
    _, ins, ref = _case(c.name, "big_logits", "nhwc_f32")
    lg = ins["ol"][..., 128:].reshape(-1, 8)
    equal = (lg == lg[:, :1]).all(1)
    assert int(equal.sum()) >= max(1, lg.shape[0] // 5)
    assert bool((ref.aw.reshape(-1, 8)[equal] == 0.125).all())
    assert bool((lg[~equal] == 88.0).any(1).all()) and float((lg.amax(1) - lg.amin(1)).max()) > 100.0
    _, pins, _ = _case(c.name, "random", "pts_per_sample")
    assert bool((pins["ref_pts"] < 0).any()) and bool((pins["ref_pts"] > 1).any())
    assert _case(c.name, "random", "pts_shared")[1]["ref_pts"].shape[0] == 1      # batch stride 0


def test_selector_conditions():
    c = R.BY_NAME["full_blocks"]
    H, W = c.H, c.W
    ins = R.make_inputs(c, "selector", V["nhwc_f32"])
    ref = R.ref_deform_attn(c, ins)
    pick = ins["target"]["pick"]
    aw = ref.aw.gather(3, pick[..., None])
    assert bool((aw == 1.0).all()) and bool((ref.aw.sum(-1) == 1.0).all())
    px, py = ref.px.gather(3, pick[..., None])[..., 0], ref.py.gather(3, pick[..., None])[..., 0]
    tx, ty = ins["target"]["tx"], ins["target"]["ty"]
    inx, iny = (tx >= 0) & (tx < W), (ty >= 0) & (ty < H)
    assert torch.equal(px[inx], tx[inx].double()) and torch.equal(py[iny], ty[iny].double())
    assert bool(((px[~inx] == -0.5) | (px[~inx] == W - 0.5)).all()) and bool(((py[~iny] == -0.5) | (py[~iny] == H - 0.5)).all())
    # the same positions in float32, operation by operation
    off = ins["ol"][..., :128].reshape(c.B, H * W, 8, 8, 2)
    pts = R.grid_points(ins["ref_x"], ins["ref_y"])
    for a, n in ((0, W), (1, H)):
        l = (pts[..., a].view(1, -1, 1, 1) + off[..., a] / torch.tensor(float(H))).clamp(0.0, 1.0)
        p32 = (((l * 2.0 - 1.0) + 1.0) * float(n) - 1.0) / 2.0
        assert p32.dtype == torch.float32
        assert torch.equal(p32.gather(3, pick[..., None])[..., 0].double(), (px, py)[a])
    both = inx & iny
    for cond in (both & (tx == 0), both & (tx == W - 1), both & (ty == 0), both & (ty == H - 1),   # the four borders
                 both & (tx > 0) & (tx < W - 1) & (ty > 0) & (ty < H - 1),
                 tx < 0, tx >= W, ty < 0, ty >= H, ~inx & ~iny):                                     # reached by the clamp
        assert bool(cond.any())
    pix, scale = R.selector_expectation(c, ins)
    assert set(scale.unique().tolist()) == {1.0, 0.5, 0.25} and int(pix.min()) == 0 and int(pix.max()) == H * W - 1
    # unclamped (token, head)s return a value row verbatim
    out = R.selector_rows(c, ins).reshape(c.B, H * W, 8, 32)
    v = ins["value"].reshape(c.B, H * W, 8, 32)
    b, t, h = both.nonzero(as_tuple=True)
    assert torch.equal(out[b, t, h], v[b, pix[b, t, h], h])


# ----------------------------------------------------------------------------------------------------------------------
# planted errors
# ----------------------------------------------------------------------------------------------------------------------
def _hits(plant):
    hits = {}
    for c in R.CASES:
        for kind in R.KINDS[:1]:
            for v in R.VARIANTS:
                _, ins, ref = _case(c.name, kind, v.name)
                try:
                    bad = R.ref_deform_attn(c, ins, plant=plant)
                except R.NotExercised:
                    continue
                got = bad.out if (not v.bf16 or plant == "bf16_truncated") else R.bf16_rn(bad.out)
                hits["%s/%s/%s" % (c.name, kind, v.name)] = _rejected(lambda: R.check(got, ref.out, ref.bound))
    return hits


@pytest.mark.parametrize("plant", R.CORE_PLANTS)
def test_plant_is_rejected(plant):
    hits = _hits(plant)
    assert hits and any(hits.values()), plant
    caught = {k for k, v in hits.items() if v}
    print("%s: rejected on %d of %d exercised (case, kind, variant)s" % (plant, len(caught), len(hits)))
    cases = {k.split("/")[0] for k in caught}
    variants = {k.split("/")[2] for k in hits}
    if plant == "offset_y_over_W":
        assert not any(k.startswith(("one_token", "odd_9")) for k in hits) and len(cases) == 5
    if plant in ("align_corners", "logits_of_next_head", "border_padding", "no_clamp"):
        assert len(cases) == len(R.CASES)
    if plant == "ref_xy_swapped":
        assert cases >= {c.name for c in R.CASES} - {"one_token"}
    if plant in ("token_bias_not_on_logits", "token_bias_by_global_row"):
        assert variants == {v.name for v in R.VARIANTS if v.bias}
    if plant == "token_bias_by_global_row":
        assert cases == {c.name for c in R.CASES if c.B > 1}
    if plant == "head_major_read_as_nhwc":
        assert variants == {v.name for v in R.VARIANTS if v.layout == "hm"} and len(cases) == len(R.CASES) - 1
    if plant == "odd_tail_takes_previous_token":
        assert {k.split("/")[0] for k in hits} == {"odd_9", "odd_105_wide"} == cases and all(hits.values())
    if plant == "second_sample_reads_first":
        assert variants == {"pts_per_sample"} and cases == {c.name for c in R.CASES if c.B > 1}
    if plant == "bf16_truncated":
        assert variants == {v.name for v in R.VARIANTS if v.bf16} and all(hits.values())


def test_selector_plants_are_rejected_by_plain_inequality():
    c = R.BY_NAME["full_blocks"]
    seen = set()
    for v in SEL_VARIANTS:
        ins = R.make_inputs(c, "selector", v)
        want = R.selector_rows(c, ins)
        for plant in R.CORE_PLANTS:
            if plant == "bf16_truncated":   # every selector output is a bf16 number already
                continue
            try:
                bad = R.ref_deform_attn(c, ins, plant=plant).out
            except R.NotExercised:
                continue
            got = R.bf16_rn(bad) if v.bf16 else bad
            assert not torch.equal(got.to(want.dtype), want), (plant, v.name)
            seen.add(plant)
    assert seen >= {"offset_y_over_W", "align_corners", "no_clamp", "border_padding", "ref_xy_swapped", "logits_of_next_head",
                    "head_major_read_as_nhwc"}


def test_unknown_plant_is_an_error():
    c, ins, _ = _case("odd_9", "random", "nhwc_f32")
    with pytest.raises(ValueError):
        R.ref_deform_attn(c, ins, plant="no_such_plant")
    with pytest.raises(ValueError):
        R.ref_deform_attn(c, ins, plant="pos_by_global_row")
    x, pos = R.make_add_pos_inputs(3, 1, False)
    with pytest.raises(ValueError):
        R.ref_add_pos(x, pos, plant="align_corners")


# ----------------------------------------------------------------------------------------------------------------------
# the non-finite test's problem
# ----------------------------------------------------------------------------------------------------------------------
def test_nudged_positions_keep_off_the_kinks_and_non_finite_sets_match_grid_sample():
    c = R.BY_NAME["wide"]
    ins = R.make_inputs(c, "nudged", V["nhwc_f32"])
    ref = R.ref_deform_attn(c, ins)
    for p, raw in ((ref.px, ref.raw_x), (ref.py, ref.raw_y)):
        fr = p - p.floor()
        assert bool(((fr >= 0.015) & (fr <= 0.985)).all())
        assert bool(((raw.abs() >= 5e-5) & ((raw - 1.0).abs() >= 5e-5)).all())
    assert float(ref.aw.min()) > 1e-9
    B, H, W = c.B, c.H, c.W
    for bad in (float("nan"), float("inf")):
        for (b, y, x) in ((1, 4, 6), (0, 0, 0), (1, H - 1, W - 1)):
            val = ins["value"].clone()
            val[b, y, x, 3 * 32 + 5] = bad
            r = R.ref_deform_attn(c, dict(ins, value=val))
            want = R.grid_sample_composition(val.double().reshape(B, H * W, 256), ins["ol"].double().reshape(B, H * W, 192),
                                             _points(c, ins), H, W).reshape(B, H, W, 256)
            nf = ~torch.isfinite(r.out)
            assert torch.equal(nf, ~torch.isfinite(want)) and 0 < int(nf.sum()) < 200
            assert bool(torch.isfinite(r.bound[~nf]).all())
            assert bool((nf.nonzero()[:, 0] == b).all()) and bool((nf.nonzero()[:, 3] == 3 * 32 + 5).all())


# ----------------------------------------------------------------------------------------------------------------------
# add_pos
# ----------------------------------------------------------------------------------------------------------------------
def test_add_pos_reference_and_plants():
    for T in R.ADD_POS_ROWS:
        for B in R.ADD_POS_B:
            for bf in (False, True):
                x, pos = R.make_add_pos_inputs(T, B, bf)
                want = R.ref_add_pos(x, pos)
                assert want.dtype == x.dtype and want.shape == x.shape
                s64 = x.double() + pos.double()[None]
                ok = torch.isfinite(s64)
                if bf:   # one rounding of the exact sum of a bf16 and an fp32 number would differ from two: fp32 first
                    assert torch.equal(want.double()[ok], R.bf16_rn((x.float() + pos[None]).double())[ok])
                    assert want[0, 0, 5:8].tolist() == [1.0, 1.0 + 2.0 ** -6, -3.0 - 2.0 ** -5]     # the ties, to even
                else:
                    assert float((want.double() - s64)[ok].abs().max()) <= R.U32 * float(s64[ok].abs().max())
                assert int(torch.isnan(want).sum()) >= 3 and int(torch.isinf(want).sum()) >= 1
                assert R.same_bits(want, want.clone()) and not R.same_bits(want, torch.nan_to_num(want.float(), nan=1.0))
                for plant in R.ADD_POS_PLANTS:
                    try:
                        bad = R.ref_add_pos(x, pos, plant=plant)
                    except R.NotExercised:
                        assert (plant == "pos_by_global_row" and B == 1) or (plant == "bf16_truncated" and not bf)
                        continue
                    assert not R.same_bits(bad, want), (plant, T, B, bf)
