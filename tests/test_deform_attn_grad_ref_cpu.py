"""tests/deform_attn_grad_ref.py on its own, without a GPU: the closed-form backward is fp64 autograd of the F.grid_sample
composition, a float32 / int64 emulation of the three kernels of csrc/deform_grad.hip sits inside every derived bound, the
`exact` kind is exact, no case is vacuous, the share of widened points stays under its cap, and every planted error is
rejected."""
import functools

import pytest
import torch

import deform_attn_grad_ref as R
from deform_attn_ref import grid_sample_composition

_id = lambda c: c.name  # noqa: E731


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@functools.lru_cache(maxsize=None)
def _case(name, kind, pts):
    c = R.BY_NAME[name]
    ins = R.make_grad_inputs(c, kind, pts)
    return c, ins, R.ref_deform_grad(c, ins)


def _autograd(c, ins):
    B, N = c.B, c.H * c.W
    v = ins["value"].double().requires_grad_(True)
    o = ins["ol"].double().requires_grad_(True)
    out = grid_sample_composition(v, o, ins["ref_pts"].double().expand(B, N, 2), c.H, c.W)
    (out * ins["d_out"].double()).sum().backward()
    return v.grad, o.grad


# ----------------------------------------------------------------------------------------------------------------------
# the closed form is the backward of the operation
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", R.PTS)
@pytest.mark.parametrize("c", R.GCASES, ids=_id)
def test_closed_form_is_fp64_autograd_on_nudged(c, pts):
    """Both sides are fp64: 1e-10 of max|ref| per output (at most 10^5 terms rounded at 2^-53 stay far below it)."""
    _, ins, ref = _case(c.name, "nudged", pts)
    dv, dol = _autograd(c, ins)
    assert ref.d_value.shape == dv.shape and ref.d_ol.shape == dol.shape
    for got, want in ((ref.d_value, dv),) + tuple(zip(R.split_ol(ref.d_ol), R.split_ol(dol))):
        assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max()), (c.name, pts)
    assert float(ref.d_ol[..., :128].abs().max()) > 0 or c.name == "one_token"


@pytest.mark.parametrize("pts", R.PTS)
@pytest.mark.parametrize("name", R.EXACT_CASES)
def test_exact_kind_is_exact(name, pts):
    """Kinks (integer px), clamp edges (raw exactly 0 or 1) and out-of-image targets: the closed form's conventions are
    autograd's.  The six points at logit -200 weigh 1.4e-87 in fp64 and 0 in fp32, so both sides are compared as fp32
    numbers, exactly; the emulation of the kernels returns the same bits."""
    c, ins, ref = _case(name, "exact", pts)
    dv, dol = _autograd(c, ins)
    assert torch.equal(ref.d_value.float(), dv.float()) and torch.equal(ref.d_ol.float(), dol.float())
    for contract in (False, True):
        ev, eo = R.emulate_f32(c, ins, contract)
        assert torch.equal(ev, ref.d_value.float()) and torch.equal(eo, ref.d_ol.float())
        assert torch.equal(ev.double(), ref.d_value.float().double())
    # the conventions are met: the two chosen points of every (token, head)
    t = ins["target"]
    H, W = c.H, c.W
    pick = t["pick"]
    px, py = ref.px.gather(3, pick), ref.py.gather(3, pick)
    rx, ry = ref.raw_x.gather(3, pick), ref.raw_y.gather(3, pick)
    tx2, ty2 = t["tx2"], t["ty2"]
    assert bool((ref.aw.gather(3, pick) == 0.5).all())
    for t2, p, raw, n in ((tx2, px, rx, W), (ty2, py, ry, H)):
        centre = (t2 >= 0) & (t2 <= 2 * n - 2)
        assert torch.equal(p[centre], t2[centre].double() / 2) and bool((p[centre] == p[centre].floor()).all())
        assert bool((t2 == 2 * n - 2).any()) and bool((t2 == 0).any())                 # the last cell: 2nd tap outside
        assert bool((raw[t2 == -1] == 0.0).all()) and bool((raw[t2 == 2 * n - 1] == 1.0).all())
        assert bool((t2 == -1).any()) and bool((t2 == 2 * n - 1).any())
        assert bool((raw[t2 < -1] < 0).all()) and bool((raw[t2 > 2 * n - 1] > 1).all())
        assert bool((t2 < -1).any()) and bool((t2 > 2 * n - 1).any())
    on_edge, outside = R.exact_edge_sets(c, ins)
    dox = ref.d_ol[..., :128].reshape(c.B, H * W, 8, 8, 2)
    assert bool((dox[outside] == 0).all()) and int(outside.sum()) > 100
    assert int((dox[on_edge] != 0).sum()) * 2 > int(on_edge.sum()) > 100


# ----------------------------------------------------------------------------------------------------------------------
# the emulation of the kernels stays inside the bound; widened points are rare
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts", R.PTS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", R.GCASES, ids=_id)
def test_emulation_is_inside_the_bound(c, kind, pts):
    _, ins, ref = _case(c.name, kind, pts)
    for t in (ref.bound_value, ref.bound_ol):
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()) and bool((t >= 0).all())
    assert bool((ref.bound_value > 0).all())
    assert ref.widened < R.WIDENED_CAP, ref.widened
    for contract in (False, True):
        ev, eo = R.emulate_f32(c, ins, contract)
        tag = "%s.%s.%s.%s" % (c.name, kind, pts, "fma" if contract else "mul_add")
        R.check(ev, ref.d_value, ref.bound_value, tag + ".d_value")
        for part, got, want, bound in zip(("d_offsets", "d_logits"), R.split_ol(eo), R.split_ol(ref.d_ol), R.split_ol(ref.bound_ol)):
            R.check(got, want, bound, tag + "." + part)
        if not contract:
            print("emulation %s widened %.2e | bound/max, error/bound: d_value %.2e %.3f  d_offsets %.2e %.3f  d_logits %.2e %.3f"
                  % ((tag, ref.widened, float(ref.bound_value.max() / ref.d_value.abs().max()),
                      R.error_over_bound(ev, ref.d_value, ref.bound_value))
                     + tuple(x for got, want, bound in zip(R.split_ol(eo), R.split_ol(ref.d_ol), R.split_ol(ref.bound_ol))
                             for x in (float(bound.max() / want.abs().max().clamp_min(1e-300)), R.error_over_bound(got, want, bound)))))


def test_widened_points_widen_the_bound():
    """A position put exactly on a kink and a location put exactly on the clamp edge: the bound there covers both sides."""
    c = R.BY_NAME["pow2"]
    ins = R.make_grad_inputs(c, "exact", "shared")
    ref = R.ref_deform_grad(c, ins)
    assert ref.widened > 0.1
    left = R.ref_deform_grad(c, ins, plant="left_derivative_at_kink", bounds=False)
    excl = R.ref_deform_grad(c, ins, plant="clamp_mask_exclusive", bounds=False)
    for other in (left, excl):
        assert not torch.equal(other.d_ol, ref.d_ol)
        assert bool(((other.d_ol - ref.d_ol).abs() <= ref.bound_ol).all())


# ----------------------------------------------------------------------------------------------------------------------
# no case is vacuous
# ----------------------------------------------------------------------------------------------------------------------
def test_case_table():
    rows = {c.name: c.B * c.H * c.W for c in R.GCASES}
    assert [c.name for c in R.GCASES] == ["one_token", "odd_9", "odd_105_wide", "tall", "wide", "full_blocks", "very_wide",
                                          "tiles_2x3", "pow2"]
    assert (rows["one_token"], rows["odd_9"], rows["odd_105_wide"]) == (1, 9, 105)          # odd rows: the tail half-wave
    assert rows["odd_9"] % 8 == 1 and rows["very_wide"] % 8 == 2                              # ... and waves wholly past the end
    t = R.BY_NAME["tiles_2x3"]
    assert (t.B, t.H, t.W) == (2, 19, 35) and t.H > R.TS and t.H % R.TS and t.W > 2 * R.TS and t.W % R.TS
    p = R.BY_NAME["pow2"]
    assert (p.B, p.H, p.W) == (2, 8, 16)
    assert {c.name for c in R.GCASES if c.H != c.W} >= {"tall", "wide", "very_wide", "tiles_2x3", "pow2", "odd_105_wide"}
    assert R.fx_bits(8192) == 49 and R.fx_bits(4096) == 50 and R.fx_bits(1) == 50
    assert R.fx_exponents(torch.tensor([[[0.0]], [[1.0]], [[0.75]], [[float("inf")]]])) == [0, 1, 0, 0]


@pytest.mark.parametrize("c", R.GCASES, ids=_id)
def test_case_conditions(c):
    for pts in R.PTS:
        _, ins, ref = _case(c.name, "random", pts)
        assert ins["ref_pts"].shape[0] == (1 if pts == "shared" else c.B)
        clamped = ~(ref.mask_x & ref.mask_y)
        assert bool(clamped.any()) and (bool((~clamped).any()) or c.name == "one_token")
        if c.name in ("very_wide", "tiles_2x3"):
            assert ref.n_far > 0                                   # the out-of-window path: straight global adds
        else:
            assert c.W <= R.TS + R.RAD and c.H <= R.TS + R.RAD and ref.n_far == 0
    if c.B > 1:
        _, ins, _ = _case(c.name, "skewed", "shared")
        assert R.fx_exponents(ins["d_out"])[1] < R.fx_exponents(ins["d_out"])[0] - 40
    _, ins, ref = _case(c.name, "big_logits", "shared")
    assert float(ref.aw.max()) == 1.0 and float(ref.aw.min()) < 1e-30


# ----------------------------------------------------------------------------------------------------------------------
# planted errors
# ----------------------------------------------------------------------------------------------------------------------
def _hits(plant):
    hits = {}
    for c in R.GCASES:
        for kind in ("random", "skewed") + (("exact",) if c.name in R.EXACT_CASES else ()):
            for pts in R.PTS:
                _, ins, ref = _case(c.name, kind, pts)
                try:
                    bad = R.ref_deform_grad(c, ins, plant=plant, bounds=False)
                except R.NotExercised:
                    continue
                if kind == "exact":   # compared bit for bit, as the GPU test does: on a kink the bound covers both sides
                    hit = not (torch.equal(bad.d_value.float(), ref.d_value.float())
                               and torch.equal(bad.d_ol.float(), ref.d_ol.float()))
                else:
                    hit = (_rejected(lambda: R.check(bad.d_value, ref.d_value, ref.bound_value))
                           or _rejected(lambda: R.check(bad.d_ol, ref.d_ol, ref.bound_ol)))
                hits["%s/%s/%s" % (c.name, kind, pts)] = hit
    return hits


@pytest.mark.parametrize("plant", R.PLANTS)
def test_plant_is_rejected(plant):
    hits = _hits(plant)
    assert hits and any(hits.values()), plant
    caught = {k for k, v in hits.items() if v}
    print("%s: rejected on %d of %d exercised (case, kind, points)s" % (plant, len(caught), len(hits)))
    cases = {k.split("/")[0] for k in caught}
    tried = {k.split("/")[0] for k in hits}
    non_square = {c.name for c in R.GCASES if c.H != c.W}
    if plant in ("doffx_without_W_over_H", "doffy_times_W_over_H", "offset_y_over_W", "dvalue_cell_index_H_W_swapped"):
        assert tried == non_square == cases
    if plant in ("clamp_mask_exclusive", "left_derivative_at_kink"):
        assert {k.split("/")[1] for k in caught} == {"exact"} and cases == set(R.EXACT_CASES)
    if plant in ("clamp_mask_ignored", "border_padding_in_derivative", "dlogit_without_mean_term", "logits_of_next_head"):
        assert cases == {c.name for c in R.GCASES}
    if plant == "second_sample_reads_first_ref":
        assert all(k.endswith(("/random/per_sample", "/skewed/per_sample")) for k in hits)
        assert cases == {c.name for c in R.GCASES if c.B > 1}
    if plant == "dvalue_far_taps_dropped":
        assert tried == cases == {"very_wide", "tiles_2x3"}
    if plant == "odd_tail_takes_previous_token":
        assert tried == cases == {"odd_9", "odd_105_wide"} and all(hits.values())
    if plant == "scale_from_whole_batch":
        # (`random` samples may differ by one binade: that step is still below the fp32 terms of the bound)
        assert {k.split("/")[1] for k in caught} == {"skewed"} and cases == {c.name for c in R.GCASES if c.B > 1}


def test_unknown_plant_is_an_error():
    c, ins, _ = _case("odd_9", "random", "shared")
    with pytest.raises(ValueError):
        R.ref_deform_grad(c, ins, plant="no_such_plant")


# ----------------------------------------------------------------------------------------------------------------------
# the token subset and the d_out override used by the GPU tests
# ----------------------------------------------------------------------------------------------------------------------
def test_token_subset_rows_are_the_full_reference_rows():
    c, ins, ref = _case("wide", "random", "per_sample")
    tok = torch.tensor([0, 5, 77, c.H * c.W - 1])
    sub = R.ref_deform_grad(c, ins, tokens=tok)
    assert torch.equal(sub.d_ol, ref.d_ol[:, tok]) and torch.equal(sub.bound_ol, ref.bound_ol[:, tok])
    rest = R.ref_deform_grad(c, ins, tokens=torch.tensor([t for t in range(c.H * c.W) if t not in tok.tolist()]))
    assert float((sub.d_value + rest.d_value - ref.d_value).abs().max()) <= 1e-12 * float(ref.d_value.abs().max())
    assert torch.equal(sub.n_adds + rest.n_adds, ref.n_adds)


def test_power_of_two_scaling_commutes_in_the_emulation():
    """d_out 2^k, k = +-60: no intermediate of the three kernels under- or overflows, so every bit scales."""
    c, ins, _ = _case("tiles_2x3", "random", "shared")
    ev, eo = R.emulate_f32(c, ins, False)
    for k in (-60, 60):
        sv, so = R.emulate_f32(c, ins, False, d_out=ins["d_out"] * 2.0 ** k)
        assert torch.equal(sv, ev * 2.0 ** k) and torch.equal(so, eo * 2.0 ** k)
        assert bool(((sv != 0) == (ev != 0)).all()) and bool(((so != 0) == (eo != 0)).all()) and bool(torch.isfinite(sv).all())


def test_outlier_grows_only_its_samples_step():
    c, ins, ref = _case("tiles_2x3", "random", "shared")
    d_out = ins["d_out"].clone()
    d_out[1, 300, 77] = 2.0 ** 20 * float(d_out.abs().max())
    big = R.ref_deform_grad(c, ins, d_out=d_out)
    assert torch.equal(big.bound_value[0], ref.bound_value[0]) and torch.equal(big.d_value[0], ref.d_value[0])
    e0, e1 = R.fx_exponents(ins["d_out"]), R.fx_exponents(d_out)
    assert e1[0] == e0[0] and e1[1] == e0[1] + 20
    for contract in (False, True):
        ev, eo = R.emulate_f32(c, ins, contract, d_out=d_out)
        R.check(ev, big.d_value, big.bound_value, "outlier d_value")
        R.check(eo, big.d_ol, big.bound_ol, "outlier d_ol")
