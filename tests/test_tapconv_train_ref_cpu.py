"""The reference helper of the tap-list training unit (tests/tapconv_train_ref.py), checked on the CPU for every case
the GPU file runs: the ReLU band holds at most 5 % of the elements with the reference alone, the hand-written chain
equals the autograd reference in fp64, the live-tap rule agrees with camera_branch_ref's, and every planted error in a
reference copy exceeds the bound the GPU tests apply - so the bound has teeth before a kernel is involved."""
import pytest
import torch

import camera_branch_ref as CB
import tapconv_train_ref as R


def _stand_in_mask(op):
    """No kernel here: the mask both sides share is the one of the rounding-emulated forward."""
    return (R.evaluate(op, None, emulate=True)["y"] > 0).double() if op["relu"] else None


@pytest.mark.parametrize("u", R.UNITS, ids=lambda u: u.name)
def test_band_reference_equals_hand_chain_and_floor(u):
    op = R.make_operands(u)
    mask = _stand_in_mask(op)
    ref = R.reference(op, mask)
    if op["relu"]:
        frac, _ = R.band_fraction(R.reference(op))   # the reference alone
        print("band %-20s %.2f %%" % (u.name, 100 * frac))
        assert frac <= R.T.BAND_MAX_FRACTION, frac
    exact = R.evaluate(op, mask, emulate=False)
    for k, (em, el) in R.floors(ref, exact).items():
        assert max(em, el) < 1e-9, (k, em, el)
    if u.conv_bias:
        assert float(ref["db"].abs().max()) < 1e-9 * float(ref["dbeta"].abs().max())   # the BatchNorm removes the bias
    floor = R.floors(ref, R.evaluate(op, mask, emulate=True))
    assert {"z", "y", "dz", "g1", "dw", "dgamma", "dbeta", "running_mean", "running_var"} <= set(floor)
    for k, fl in sorted(floor.items()):
        print("floor %-20s %-13s max %.3e l2 %.3e" % (u.name, k, fl[0], fl[1]))
        assert max(fl) < 2e-2, (k, fl)


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_by_taps_equals_autograd(case):
    if case[3] * case[4] > 256 * 256:
        case = case[:3] + (64, 64) + case[5:]        # the production shapes at 64 channels: the tap geometry is the same
    x, dy = R.make_wgrad_operands(case)
    ref = R.wgrad_reference(x, dy, case[5], case[6])
    got = R.wgrad_by_taps(x, dy, case[5], case[6])
    assert max(R.errors(got, ref)) < 1e-12
    dead = sorted(set(range(case[5] ** 2)) - set(R.live_taps(case[1], case[2], case[5], case[6])))
    assert float(ref.reshape(*ref.shape[:2], -1)[:, :, dead].abs().max() if dead else 0.0) == 0.0


def test_live_taps_agree_with_camera_branch_ref():
    for H, W in ((1, 1), (5, 9), (8, 22), (3, 5), (16, 44)):
        for d in (1, 2, 4, 6, 9, 12, 24, 36):
            assert R.live_taps(H, W, 3, d) == CB.live_taps(H, W, 3, d), (H, W, d)
        assert R.live_taps(H, W, 1, 1) == CB.live_taps(H, W, 1, 1) == [0]
    assert len(R.live_taps(8, 22, 3, 2)) == 9 and R.live_taps(8, 22, 3, 12) == [3, 4, 5]
    assert R.live_taps(8, 22, 3, 24) == R.live_taps(8, 22, 3, 36) == [4]


# plant -> (the weight-gradient case that exposes it); the last two live in the unit
WGRAD_PLANTS = {
    "tap_from_neighbour_image": (3, 5, 9, 128, 64, 3, 4),
    "row_wrap": (3, 5, 9, 128, 64, 3, 4),
    "dead_tap_nonzero": (2, 5, 9, 64, 128, 3, 6),
    "ky_kx_swapped": (2, 5, 9, 64, 64, 3, 1),
    "dilation_ignored": (3, 5, 9, 128, 64, 3, 4),
    "last_partial_block_dropped": (2, 5, 9, 64, 64, 3, 1),
}
UNIT_PLANTS = {"img_bias_wrong_image": ("k1_img_bias", "dbias"), "dgrad_unflipped": ("k3_d2", "g1")}


def test_every_plant_is_listed():
    assert set(WGRAD_PLANTS) | set(UNIT_PLANTS) == set(R.PLANTS)
    assert all(c in R.WGRAD_CASES for c in WGRAD_PLANTS.values())


@pytest.mark.parametrize("plant", sorted(WGRAD_PLANTS))
def test_planted_wgrad_errors_are_rejected(plant):
    """The kernel test's bound on dw alone (no rounding between the bf16 operands and the fp32 result: the floor is 0
    and the bound is the fp32 minimum) rejects each wrong weight gradient."""
    case = WGRAD_PLANTS[plant]
    x, dy = R.make_wgrad_operands(case)
    ref = R.wgrad_reference(x, dy, case[5], case[6])
    bad = R.wgrad_by_taps(x, dy, case[5], case[6], plant=plant)
    em, el = R.errors(bad, ref)
    print("plant %-28s max %.3e l2 %.3e" % (plant, em, el))
    assert em > R.T.MIN_F32 and el > R.T.MIN_F32


@pytest.mark.parametrize("plant", sorted(R.PLANTS))
def test_planted_unit_errors_are_rejected(plant):
    """The same plants inside the unit: the bound of the node test (3 x floor, the minima) rejects them."""
    name, key = UNIT_PLANTS.get(plant, ("k3_d6" if plant == "dead_tap_nonzero" else "k3_d2", "dw"))
    if plant == "dilation_ignored":
        name = "k3_d4_norelu"
    u = next(v for v in R.UNITS if v.name == name)
    op = R.make_operands(u)
    mask = _stand_in_mask(op)
    ref = R.reference(op, mask)
    bound = R.bounds(R.floors(ref, R.evaluate(op, mask, emulate=True)))
    bad = R.evaluate(op, mask, emulate=True, plant=plant)
    em, el = R.errors(bad[key], ref[key])
    print("plant %-28s %-5s max %.3e (bound %.3e) l2 %.3e (bound %.3e)" % (plant, key, em, bound[key][0], el, bound[key][1]))
    assert em > bound[key][0] and el > bound[key][1]
