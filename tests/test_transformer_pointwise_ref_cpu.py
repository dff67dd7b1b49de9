"""CPU checks of tests/transformer_pointwise_ref.py itself: the numpy Philox mask against published and committed known
answers, its keep rate, the float32 emulations of the four kernels inside the derived bounds, and every planted error
outside them."""
import math

import pytest
import torch

import transformer_pointwise_ref as P

_hex = lambda ws: " ".join("%08x" % int(w) for w in ws)  # noqa: E731


def test_philox_known_answers():
    assert _hex(P.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _hex(P.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(P.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) \
        == "d16cfe09 94fdcceb 5001e420 24126ea1"


@pytest.mark.parametrize("p,thr,bits", [
    (0.1, 6554, "1111111111111111111111111111110111111111111111101111100110111111"),
    (0.5, 32768, "1110010101000100111110111110010100110111010011001100000110101110")])
def test_mask_known_answers(p, thr, bits):
    assert P.threshold(p)[0] == thr
    keep = P.keep_mask((64,), p, P.KEY, P.STREAM)
    assert "".join("1" if k else "0" for k in keep.tolist()) == bits
    # a prefix of a longer tensor is the same mask (the index is the linear element index), in any shape
    assert torch.equal(P.keep_mask((5, 64), p).view(-1)[:64], keep)
    # the seed tensor the kernels read carries the same two words
    assert P.seed_words(P.seed_tensor()) == (P.KEY, P.STREAM)


@pytest.mark.parametrize("n", [257 * 1024, 4551 * 256])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(n, p):
    thr, p_eff, scale = P.threshold(p)
    dropped = n - int(P.keep_mask((n,), p).sum())
    z = (dropped - n * p_eff) / math.sqrt(n * p_eff * (1.0 - p_eff))
    print("n %d p %.1f dropped %d z %.3f" % (n, p, dropped, z))
    assert abs(z) <= 5.0
    assert abs(z) <= 1.6          # what the reference gives on this seed: a regression check of the helper
    assert scale == pytest.approx(1.0 / (1.0 - p_eff), rel=2.0 ** -24)


def test_plants_move_the_mask():
    base = P.keep_mask((4096,), 0.5)
    for plant in ("mask_shifted_one_call", "pieces_swapped"):
        other = P.keep_mask((4096,), 0.5, plant=plant)
        assert 0.4 < float((other != base).float().mean()) < 0.6, plant
    assert torch.equal(P.keep_mask((4096,), 0.5, plant="mask_shifted_one_call")[:-8], base[8:])


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _finite(out, got):
    """The elements `check` looks at: everything but the ones whose reference overflows bf16 (those must be inf)."""
    ok = ~out.overflow
    assert bool(torch.isinf(got.double()[out.overflow]).all())
    return got.double()[ok], out.ref[ok], out.bound[ok]


# ----------------------------------------------------------------------------------------------------------------------
# GELU + dropout
# ----------------------------------------------------------------------------------------------------------------------
SMALL_GELU = [s for s in P.GELU_SHAPES if s[0] * s[1] <= 257 * 1024]


@pytest.mark.parametrize("shape", SMALL_GELU, ids=str)
@pytest.mark.parametrize("p", P.PS)
def test_gelu_dropout_emulation_is_inside_the_bounds(shape, p):
    h, dy = P.make_gelu_inputs(*shape)
    m = P.multiplier(shape, p)
    scale = P.threshold(p)[2] if p else 1.0
    fwd = P.ref_gelu_dropout(h, m, scale)
    P.check(*_finite(fwd, P.emu_gelu_dropout(h, m)), "y")
    bwd = P.ref_gelu_dropout_bwd(h, dy, m)
    got = P.emu_gelu_dropout_bwd(h, dy, m)
    P.check(*_finite(bwd, got), "dh")
    assert bool(torch.isfinite(got.double()[~bwd.overflow]).all())
    # +-3e38: derivative 1 or 0, not NaN
    big = h.double().abs() > 1e38
    assert bool(big.any()) and not bool(torch.isnan(got.double()[big]).any())
    # dropped elements are exactly zero in both directions
    if p:
        assert not bool(P.emu_gelu_dropout(h, m).double()[m == 0].any()) and not bool(got.double()[m == 0].any())


def test_exp_cap_is_not_what_carries_the_bound():
    """EXP_REL = 2^-21 is a condition on v_exp_f32; on the grid it adds at most 2^-21 |v phi(v)| <= 1.4e-7 to E_d, below
    the erf formula's 1.5e-7 share and three orders below half a bf16 ulp of d."""
    v = torch.linspace(-12, 12, 4001, dtype=torch.float64)
    assert float((v.abs() * P.phi64(v)).max()) * P.EXP_REL < 1.5e-7


@pytest.mark.parametrize("plant", ["mask_not_applied_in_backward", "scale_dropped", "mask_shifted_one_call",
                                   "pieces_swapped", "tanh_gelu_derivative"])
def test_gelu_dropout_plant_is_rejected(plant):
    shown = 0
    for shape in SMALL_GELU:
        for p in (0.1, 0.5):
            h, dy = P.make_gelu_inputs(*shape)
            m, scale = P.multiplier(shape, p), P.threshold(p)[2]
            fwd, bwd = P.ref_gelu_dropout(h, m, scale), P.ref_gelu_dropout_bwd(h, dy, m)
            if plant in ("mask_not_applied_in_backward", "tanh_gelu_derivative"):
                bad_y, bad_dh = P.emu_gelu_dropout(h, m), P.emu_gelu_dropout_bwd(h, dy, m, plant=plant)
                assert not _rejected(lambda: P.check(*_finite(fwd, bad_y)))
            else:   # a wrong multiplier in both directions
                mb = P.multiplier(shape, p, plant=plant)
                bad_y, bad_dh = P.emu_gelu_dropout(h, mb), P.emu_gelu_dropout_bwd(h, dy, mb)
                fin = ~fwd.overflow & torch.isfinite(bad_y.double())
                assert _rejected(lambda: P.check(bad_y.double()[fin], fwd.ref[fin], fwd.bound[fin])), (plant, shape, p)
            fin = ~bwd.overflow & torch.isfinite(bad_dh.double())
            assert _rejected(lambda: P.check(bad_dh.double()[fin], bwd.ref[fin], bwd.bound[fin])), (plant, shape, p)
            shown += 1
    assert shown == 2 * len(SMALL_GELU)


# ----------------------------------------------------------------------------------------------------------------------
# add + dropout + LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
SMALL_LN = [c for c in P.LN_CASES if c.rows <= 257]


def _ln_run(c, first, p, plant=None):
    res, a, dy, gamma, beta = P.make_ln_inputs(c, first)
    m = P.multiplier(res.shape, p)
    scale = P.threshold(p)[2] if p else 1.0
    mask_plant = plant if plant in ("scale_dropped", "mask_shifted_one_call", "pieces_swapped") else None
    mk = P.multiplier(res.shape, p, plant=mask_plant) if (p and mask_plant) else m
    s32 = P.emu_add(res, a, mk)
    got = P.emu_add_dropout_ln_bwd(s32, dy, gamma, P.EPS, mk, c.a_bf16, plant=None if mask_plant else plant)
    s_ref, s_bound = P.ref_add(res, a, m)
    ref = P.ref_add_dropout_ln_bwd(s32, dy, gamma, P.EPS, m, scale, c.a_bf16)
    return s32, got, s_ref, s_bound, ref, m


@pytest.mark.parametrize("c", SMALL_LN, ids=lambda c: c.name)
@pytest.mark.parametrize("p", P.PS)
def test_add_dropout_ln_emulation_is_inside_the_bounds(c, p):
    for first in P.ln_firsts(c):
        s32, (ds, da, dg, db), s_ref, s_bound, ref, m = _ln_run(c, first, p)
        P.check(s32, s_ref, s_bound, "s")
        P.check(ds, ref.ds, ref.bound_ds, "ds")
        P.check(da, ref.da, ref.bound_da, "da")
        P.check(dg, ref.dgamma, ref.bound_dgamma, "dgamma")
        P.check(db, ref.dbeta, ref.bound_dbeta, "dbeta")
        if p:
            assert not bool(da.double()[m == 0].any())


@pytest.mark.parametrize("plant", ["mask_not_applied_in_backward", "scale_dropped", "mask_shifted_one_call",
                                   "pieces_swapped", "da_before_xhat_term"])
def test_add_dropout_ln_plant_is_rejected(plant):
    for c in SMALL_LN:
        if c.rows < 4:
            continue          # a single constant row has a = 0 and xhat = 0: nothing to show
        for p in (0.1, 0.5):
            s32, (ds, da, dg, db), s_ref, s_bound, ref, m = _ln_run(c, 0, p, plant=plant)
            s_bad = _rejected(lambda: P.check(s32, s_ref, s_bound))
            da_bad = _rejected(lambda: P.check(da, ref.da, ref.bound_da))
            if plant in ("mask_not_applied_in_backward", "da_before_xhat_term"):
                assert da_bad and not s_bad, (plant, c.name, p)
            else:
                assert s_bad and da_bad, (plant, c.name, p)
