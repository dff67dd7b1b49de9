"""tests/bev_encoder_train_ref.py against torch's own fp64 autograd, its bf16 emulation against its bounds, and the
plants those bounds have to reject.  No GPU."""
import pytest
import torch

import bev_encoder_train_ref as E
import train_node_ref as R

UNITS = [(u, 3) for u in E.BIASED_3X3] + [(u, 1) for u in E.CONV_1X1]
_cache = {}


def _unit(u, k):
    """(operands, torch's fp64 unit, the reference with torch's ReLU mask) of a case, computed once."""
    if u.name not in _cache:
        op = E.make_unit_operands(u, k)
        tor = E.torch_unit(op)
        _cache[u.name] = (op, tor, E.unit_reference(op, tor["mask"]))
    return _cache[u.name]


@pytest.mark.parametrize("u,k", UNITS, ids=lambda v: getattr(v, "name", str(v)))
def test_unit_reference_is_torchs_biased_conv_bn_relu_in_fp64(u, k):
    """BN(conv(x) + b) in training mode: y and every gradient equal the bias-free formulas, running_mean carries m * b,
    and torch's own gradient of the bias is zero up to fp64 rounding (the reference holds the exact 0)."""
    op, tor, ref = _unit(u, k)
    for key in ("y", "g1", "dw", "dgamma", "dbeta", "running_mean", "running_var"):
        assert torch.allclose(ref[key], tor[key], rtol=1e-9, atol=1e-11 * float(tor[key].abs().max())), key
    assert tor["num_batches_tracked"] == 1
    assert bool((ref["dbias"] == 0).all())
    assert float(tor["dbias"].abs().max()) <= 1e-10 * float(tor["dbeta"].abs().max())
    # the second derivation (train_node_ref.evaluate without rounding) agrees too
    ev = E.unit_evaluate(op, tor["mask"], emulate=False)
    for key in E.UNIT_OUTPUTS + ("dbias",):
        assert R.errors(ev[key], ref[key])[0] <= 1e-9, key


@pytest.mark.parametrize("u,k", UNITS, ids=lambda v: getattr(v, "name", str(v)))
def test_unit_emulation_is_inside_every_bound_and_the_plants_are_not(u, k):
    op, tor, ref = _unit(u, k)
    mask = tor["mask"]
    emu = E.unit_evaluate(op, mask, emulate=True)
    bound = R.bounds(R.floors(ref, emu, E.UNIT_OUTPUTS))
    assert set(bound) == set(E.UNIT_OUTPUTS)
    for key in E.UNIT_OUTPUTS:
        e = R.errors(emu[key], ref[key])
        assert e[0] <= bound[key][0] and e[1] <= bound[key][1], (key, e, bound[key])
    assert bool((emu["dbias"] == 0).all())
    # bias values of the order of z's standard deviation
    zstd = float(ref["z"].std())
    assert 0.3 * zstd <= float(op["bias"].abs().min()) and float(op["bias"].abs().max()) <= 2.0 * zstd
    for plant in ("running_mean_without_bias", "running_mean_full_bias"):
        bad = E.unit_evaluate(op, mask, emulate=True, plant=plant)
        e = R.errors(bad["running_mean"], ref["running_mean"])
        assert e[0] > bound["running_mean"][0] and e[1] > bound["running_mean"][1], (plant, e, bound["running_mean"])
    bad = E.unit_evaluate(op, mask, emulate=True, plant="bias_grad_sum_dy")
    assert R.errors(bad["dbias"], ref["dbias"]) == (float("inf"), float("inf"))   # an exact 0 admits only an exact 0
    assert R.errors(emu["dbias"], ref["dbias"]) == (0.0, 0.0)


def test_the_ring_case_takes_its_floor_from_the_same_widths():
    small = next(u for u in E.BIASED_3X3 if u.name == E.RING_FLOOR_FROM)
    assert (small.Cx, small.Cout, small.C2, small.up) == (E.RING.Cx, E.RING.Cout, E.RING.C2, E.RING.up)


_head_cache = {}


def _head(case):
    name = case[0]
    if name not in _head_cache:
        op = E.make_head_operands(*case)
        _head_cache[name] = (op, E.head_evaluate(op))
    return _head_cache[name]


SMALL_HEAD_CASES = [c for c in E.HEAD_CASES if c[2][1] * c[2][2] < 1000] + [E.HEAD_CASES[2]]


@pytest.mark.parametrize("case", SMALL_HEAD_CASES, ids=lambda c: c[0])
def test_head_reference_is_torchs_conv_and_cross_entropy_in_fp64(case):
    op, ref = _head(case)
    tor = E.torch_head(op)
    assert set(tor) == set(ref)
    for key in ref:
        assert E.rel_max(ref[key], tor[key]) <= 1e-12, key
    if case[3]:
        t = op["t"]
        assert int(((t < 0) | (t >= op["K"])).sum()) == 6 and float(op["cw"][1]) == 0.0 and int((t == 1).sum()) > 0


@pytest.mark.parametrize("case", SMALL_HEAD_CASES, ids=lambda c: c[0])
def test_head_emulation_is_inside_every_bound_and_the_neighbour_plant_is_not(case):
    """fp32 arithmetic with dy rounded to bf16 stays inside the bounds of the 128-channel tests; a pixel sum that takes
    in the neighbouring pixel's lanes misses the logits' and the loss' bound by orders of magnitude."""
    op, ref = _head(case)
    emu = E.head_evaluate(op, dtype=torch.float32)
    for key, err in E.head_errors(emu, ref).items():
        assert err <= E.head_bound(key), (key, err)
    bad = E.head_evaluate(op, plant="neighbour_lanes")
    errs = E.head_errors(bad, ref)
    assert errs["logits"] > 1e3 * E.HEAD_BOUNDS["logits"] and errs["loss"] > 1e2 * E.HEAD_BOUNDS["loss"], errs
    assert errs["ce_dw"] > E.HEAD_BOUNDS["dw"], errs


def test_head_cases_cover_a_ragged_pass_and_a_second_grid_stride_trip():
    pixels = {c[0]: c[2][0] * c[2][1] * c[2][2] for c in E.HEAD_CASES}
    assert pixels["ragged_2x5x7_k4"] % 8 != 0                      # 8 pixels per wave pass
    assert pixels["second_trip_1x136x128_k4"] > 512 * 4 * 8        # HC_BLOCKS workgroups x 4 waves x 8 pixels
    assert {c[1] for c in E.HEAD_CASES} == {4, 8}


def test_module_rule():
    mid = torch.tensor([1.0, -4.0, 2.0])
    comp = mid + torch.tensor([0.01, 0.0, 0.0])
    ok, dn, dc, allow = E.module_within(mid + torch.tensor([0.0, 0.02, 0.0]), comp, mid)
    assert ok and dn == pytest.approx(0.02) and dc == pytest.approx(0.01) and allow == pytest.approx(0.02 + 4 * 2.0 ** -9)
    assert not E.module_within(mid + torch.tensor([0.0, 0.03, 0.0]), comp, mid)[0]
