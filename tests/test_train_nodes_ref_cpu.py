"""The reference helper of the per-node training tests (tests/train_node_ref.py), checked on the CPU for every case the
GPU file runs: the ReLU band holds at most 5 % of the elements, the hand-written chain equals the autograd reference in
fp64, the rounding-emulated chain stays within its own floor (< 2e-2), and three planted errors in a reference copy
exceed the bound the GPU tests apply - so the bound has teeth before a kernel is involved.  Floors go to the test log."""
import pytest
import torch

import train_node_ref as R

UNITS = R.FUSED + R.CONV + R.UPCONV + R.BN + [R.FUSED_VS_UNFUSED[-1], R.ZERO_GRAD, R.ONE_ROW, R.COUT32, R.SMALL_GAMMA]
BIG = 4 * 100 * 100 * 64 * 9 * 64      # cases above this many multiply-adds per conv are checked forward + floor only


def _operands(u):
    if u.name == R.DEGENERATE.name:
        return R.make_degenerate_operands()
    if u.name == R.ZERO_GRAD.name:
        return R.make_zero_grad_operands()
    if u.name == R.SMALL_GAMMA.name:
        return R.make_small_gamma_operands()
    op = R.make_operands(u)
    if u in R.CONV or u in R.UPCONV:
        op["bn"], op["relu"] = False, False
    return op


def _stand_in_mask(op):
    """No kernel here: the mask both sides share is the one of the rounding-emulated forward."""
    return (R.evaluate(op, None, emulate=True)["y"] > 0).double() if op["relu"] else None


def _log(name, floor):
    for k, (fm, fl) in sorted(floor.items()):
        print("floor %-40s %-13s max %.3e l2 %.3e" % (name, k, fm, fl))


@pytest.mark.parametrize("u", UNITS + [R.DEGENERATE], ids=lambda u: u.name)
def test_band_floor_and_planted_errors(u):
    op = _operands(u)
    mask = _stand_in_mask(op)
    ref = R.reference(op, mask)
    if op["relu"]:
        frac, _ = R.band_fraction(ref)
        print("band %-40s %.2f %%" % (u.name, 100 * frac))
        assert frac <= R.BAND_MAX_FRACTION, frac
    emu = R.evaluate(op, mask, emulate=True)
    floor = R.floors(ref, emu)
    _log(u.name, floor)
    for k, fl in floor.items():
        if u.name == R.DEGENERATE.name and k in ("dz", "dw"):
            continue   # the variance-0 channel carries invstd = 316: judged per channel on the GPU, see the test there
        assert max(fl) < 2e-2, (k, fl)
    if u.name in (R.DEGENERATE.name, R.ZERO_GRAD.name, R.ONE_ROW.name):
        return
    bound = R.bounds(floor)
    planted = []
    if op["bn"]:
        planted.append(("dgamma_without_mean", "dgamma"))
    if u.Cx and u.up > 1:
        planted.append(("upsample_adjoint_last_row_dropped", "g1"))
    if u.Cx:
        planted.append(("unflipped_taps", "g1"))
    for plant, key in planted:
        bad = R.evaluate(op, mask, emulate=False, plant=plant, dtype=torch.float32 if u.B * u.H * u.W * u.up ** 2
                         * (u.Cx + u.C2) * 9 * u.Cout > BIG else torch.float64)
        em, el = R.errors(bad[key], ref[key])
        print("plant %-40s %-34s %s: max %.3e (bound %.3e) l2 %.3e (bound %.3e)" % (u.name, plant, key, em, bound[key][0],
                                                                                 el, bound[key][1]))
        assert em > bound[key][0] and el > bound[key][1], (plant, key, em, el, bound[key])


@pytest.mark.parametrize("u", [x for x in UNITS if x.B * x.H * x.W <= 2 * 37 * 29] + [R.DEGENERATE], ids=lambda u: u.name)
def test_hand_written_chain_equals_autograd_in_fp64(u):
    op = _operands(u)
    mask = _stand_in_mask(op)
    ref, man = R.reference(op, mask), R.evaluate(op, mask, emulate=False)
    assert set(k for k in ref) == set(k for k in man), (sorted(ref), sorted(man))
    for k in ref:
        em, _ = R.errors(man[k], ref[k])
        assert em < 1e-9, (k, em)


@pytest.mark.parametrize("case", R.S2, ids=lambda c: c[0])
def test_stride2_reference_and_floor(case):
    name, K, B, H, W, C, Co, native = case
    op = R.make_s2_operands(name, K, B, H, W, C, Co)
    ref, man = R.reference(op), R.evaluate(op, emulate=False)
    for k in ("z", "g1", "dw"):
        assert R.errors(man[k], ref[k])[0] < 1e-9, k
    floor = R.floors(ref, R.evaluate(op, emulate=True, per_sample_bf16_dw=not native), ("z", "g1", "dw"))
    _log(name, floor)
    assert all(max(f) < 2e-2 for f in floor.values()), floor
    assert R.errors(R.evaluate(op, emulate=False, col2im_bf16=True)["g1"], ref["g1"])[0] < 1e-9   # col2im form = the conv's
    fold = R.floors(ref, R.evaluate(op, emulate=True, col2im_bf16=True), ("g1",))
    _log(name + ".col2im", fold)
    assert max(fold["g1"]) < 2e-2
    bad = R.evaluate(op, emulate=False, plant="unflipped_taps")
    bound = R.bounds(floor)
    em, el = R.errors(bad["g1"], ref["g1"])
    assert K == 1 or (em > bound["g1"][0] and el > bound["g1"][1])


@pytest.mark.parametrize("shards,relu,res,large", [c + (False,) for c in R.SPLIT_BN] + [(2, False, False, True)])
def test_split_batchnorm_operands(shards, relu, res, large):
    op = R.make_split_bn_operands(shards, relu=relu, res=res, large=large)
    mask = _stand_in_mask(op)
    ref = R.reference(op, mask)
    if relu:
        frac, _ = R.band_fraction(ref)
        print("band split_bn_%d large=%s %.2f %%" % (shards, large, 100 * frac))
        assert frac <= R.BAND_MAX_FRACTION
    z = op["z"].double()
    m = [z[2 * s:2 * s + 2].mean() for s in range(shards)]
    assert max(m) - min(m) > 0.3 or large      # the shards really differ
    if large:   # the channels hold the (mean, std) the GPU test asserts and reports on
        zc = R.make_split_bn_operands(shards, relu=relu, res=res, large=True, H=100, W=100)["z"].double()
        for k, (mu, sd) in enumerate(R.LARGE_MEAN, 1):
            got = abs(float(zc[:, k].mean())) / float(zc[:, k].std())
            # (bf16 spacing adds to the spread of the reported 300 / 2 and -2000 / 8 channels)
            assert abs(got / (abs(mu) / sd) - 1) < (0.03 if k <= R.LARGE_MEAN_ASSERTED else 0.3), (k, got)
    floor = R.floors(ref, R.evaluate(op, mask, emulate=True))
    _log("split_bn_%d_%s" % (shards, large), floor)
    assert large or all(max(f) < 2e-2 for f in floor.values()), floor


def test_mask_check_rejects_a_wrong_decision_outside_the_band():
    op = R.make_operands(R.BN[0])
    ref = R.reference(op)
    y = ref["y"].clone()
    R.mask_check(y, ref)
    i = int(ref["t"].flatten().argmax())
    y.view(-1)[i] = 0.0
    with pytest.raises(AssertionError):
        R.mask_check(y, ref)


def test_errors_of_an_all_zero_reference():
    z = torch.zeros(4)
    assert R.errors(z, z) == (0.0, 0.0)
    assert R.errors(z + 1e-30, z)[0] == float("inf")
    assert R.errors(torch.tensor([float("nan")]), torch.ones(1))[0] == float("inf")
