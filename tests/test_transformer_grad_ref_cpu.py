"""tests/transformer_grad_ref.py on its own, without a GPU: the references are torch's float64 autograd of linear /
layer_norm, a float32 emulation of each kernel's order sits inside every case's derived bound (bit equality for the
exact weight-gradient cases), the case tables cover what they must, and every planted error is rejected by `check`."""
import pytest
import torch
from torch.nn import functional as F

import transformer_grad_ref as G

_id = lambda c: c.name  # noqa: E731
SMALL_WGRAD = [c for c in G.WGRAD_CASES if c.T * c.N * c.K <= 4551 * 256 * 256]   # the 200 x 200 sample: GPU test only


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------------------------
# the references are the operations
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [G.WGRAD_BY_NAME[n] for n in ("one_past_a_block", "three_splits_ragged", "linear1")], ids=_id)
def test_wgrad_reference_is_float64_autograd_of_linear(c):
    x, dy = G.make_wgrad_inputs(c, False)
    w = torch.zeros(c.N, c.K, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c.N, dtype=torch.float64, requires_grad=True)
    F.linear(x.double(), w, b).backward(dy.double())
    ref = G.ref_wgrad(c, x, dy, False)
    assert float((ref.dw - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())
    assert float((ref.db - b.grad).abs().max()) <= 1e-12 * float(b.grad.abs().max())
    assert bool((ref.bound_dw > 0).all()) and bool((ref.bound_db > 0).all())


@pytest.mark.parametrize("rows", [1, 5, 257])
def test_layernorm_bwd_reference_is_float64_autograd_of_layer_norm(rows):
    c = G.LnbCase("ref", rows, False, False, False)
    for first in G.lnb_firsts(c):
        x, dy, gamma = G.make_lnb_inputs(c, first)
        xd = x.double().requires_grad_(True)
        gd = gamma.double().requires_grad_(True)
        bd = torch.zeros(G.C, dtype=torch.float64, requires_grad=True)
        F.layer_norm(xd, (G.C,), gd, bd, G.EPS).backward(dy.double())
        ref = G.ref_layernorm_bwd(x, dy, gamma, G.EPS, False)
        for got, want in ((ref.dx, xd.grad), (ref.dgamma, gd.grad), (ref.dbeta, bd.grad)):
            assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_what_they_must():
    shapes = {(c.T, c.N, c.K) for c in G.WGRAD_CASES}
    assert shapes >= {(1, 64, 64), (33, 64, 64), (4551, 192, 256), (4551, 256, 256), (1250, 1024, 256),
                      (1250, 256, 1024), (40000, 256, 256)}
    assert all(G.wgrad_ok(c.T, c.N, c.K) and c.T < 2 ** 18 for c in G.WGRAD_CASES)
    sp = G.wgrad_split(*G.WGRAD_BY_NAME["three_splits_ragged"][1:])
    assert sp.splits >= 3 and G.WGRAD_BY_NAME["three_splits_ragged"].T % (G.WG_TOK * sp.per) != 0
    assert G.wgrad_split(1, 64, 64) == (1, 1, 1)
    assert G.wgrad_split(40000, 256, 256) == (313, 10, 32)          # 16 tiles: 32 splits of 10 stages (the last of 3)
    assert G.wgrad_split(320000, 1024, 256).splits == 8
    assert len(G.LNB_CASES) == 32 and {c.rows for c in G.LNB_CASES} == {1, 5, 257, 4551}
    for c in G.LNB_CASES[::8]:
        kinds = set()
        for first in G.lnb_firsts(c):
            x, _, gamma = G.make_lnb_inputs(c, first)
            v = x.double().var(-1, unbiased=False)
            m = x.double().mean(-1)
            kinds |= {"constant"} if bool((v == 0).any()) else set()
            kinds |= {"offset_1000"} if bool((m > 900).any()) else set()
            kinds |= {"tiny_std"} if bool(((v > 0) & (v < 1e-2 * G.EPS)).any()) else set()
            kinds |= {"unit"} if bool(((v > 0.5) & (m.abs() < 1)).any()) else set()
        assert kinds == set(G.LNB_KINDS), (c.name, kinds)
    assert G.ln_bwd_groups(1) == 1 and G.ln_bwd_groups(5) == 2 and G.ln_bwd_groups(4551) == 911
    assert G.ln_bwd_groups(320000) <= 1024


def test_exact_grid_assertion_rejects_operands_off_the_grid():
    c = G.WGRAD_BY_NAME["one_past_a_block"]
    x, dy = G.make_wgrad_inputs(c, True)
    G._assert_exact_wgrad(x.double(), dy.double())
    for bad in ((x.double() + 1.0 / 8, dy.double()), (x.double(), dy.double() + 1.0 / 128), (x.double() * 2, dy.double())):
        with pytest.raises(AssertionError):
            G._assert_exact_wgrad(*bad)
    with pytest.raises(AssertionError):
        G.ref_wgrad(c, *G.make_wgrad_inputs(c, False), True)


# ----------------------------------------------------------------------------------------------------------------------
# float32 emulations
# ----------------------------------------------------------------------------------------------------------------------
def _wgrad_f32(c, x, dy):
    """The kernel's tree in float32: 32-token MFMA blocks per wave, the four waves, the splits, the split-order sum
    (four interleaved chains)."""
    sp = G.wgrad_split(c.T, c.N, c.K)
    xf, df = x.float(), dy.float()
    parts_w, parts_b = [], []
    for s in range(sp.splits):
        t0 = G.WG_TOK * sp.per * s
        t1 = min(c.T, t0 + G.WG_TOK * sp.per)
        waves = [torch.zeros(c.N, c.K) for _ in range(4)]
        for b0 in range(t0, t1, 32):
            waves[((b0 - t0) // 32) % 4] += df[b0:b0 + 32].t() @ xf[b0:b0 + 32]
        parts_w.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
        parts_b.append(df[t0:t1].sum(0))

    def tree(parts):
        chains = [torch.zeros_like(parts[0]) for _ in range(4)]
        for i, p in enumerate(parts):
            chains[i % 4] = chains[i % 4] + p
        return (chains[0] + chains[1]) + (chains[2] + chains[3])

    return tree(parts_w), tree(parts_b)


@pytest.mark.parametrize("exact", [False, True], ids=["randn", "exact"])
@pytest.mark.parametrize("c", SMALL_WGRAD, ids=_id)
def test_wgrad_float32_emulation_is_inside_the_bound(c, exact):
    x, dy, ref = G.wgrad_case_data(c.name, exact)
    dw, db = _wgrad_f32(c, x, dy)
    G.check(dw, ref.dw, ref.bound_dw, c.name + ".dw")
    G.check(db, ref.db, ref.bound_db, c.name + ".db")
    if exact:
        assert not ref.bound_dw.any() and not ref.bound_db.any()
        assert torch.equal(dw.double(), ref.dw) and torch.equal(db.double(), ref.db)
        assert float(ref.dw.abs().max()) > 0


@pytest.mark.parametrize("c", G.LNB_CASES, ids=_id)
def test_layernorm_bwd_float32_emulation_is_inside_the_bound(c):
    for first in G.lnb_firsts(c):
        x, dy, gamma = G.make_lnb_inputs(c, first)
        ref = G.ref_layernorm_bwd(x, dy, gamma, G.EPS, c.dx_bf16)
        dx, dg, db = G.ln_bwd_f32(x, dy, gamma, G.EPS)
        G.check(dx.bfloat16() if c.dx_bf16 else dx, ref.dx, ref.bound_dx, c.name + ".dx")
        G.check(dg, ref.dgamma, ref.bound_dgamma, c.name + ".dgamma")
        G.check(db, ref.dbeta, ref.bound_dbeta, c.name + ".dbeta")
        # the bound is a rounding bound, not a tolerance: on unit rows it stays below 1e-4 of the gradient's scale
        kind = (torch.arange(c.rows) + first) % 4
        if bool((kind == 0).any()) and not c.dx_bf16:
            assert float(ref.bound_dx[kind == 0].max()) <= 1e-4 * float(ref.dx[kind == 0].abs().max())


# ----------------------------------------------------------------------------------------------------------------------
# planted errors
# ----------------------------------------------------------------------------------------------------------------------
def _wgrad_hits(plant):
    hits = {}
    for c in SMALL_WGRAD:
        for exact in (False, True):
            x, dy, ref = G.wgrad_case_data(c.name, exact)
            try:
                bad = G.ref_wgrad(c, x, dy, exact, plant=plant)
            except G.NotExercised:
                continue
            key = "%s/%s" % (c.name, "exact" if exact else "randn")
            hits[key] = (_rejected(lambda: G.check(bad.dw, ref.dw, ref.bound_dw)),
                         _rejected(lambda: G.check(bad.db, ref.db, ref.bound_db)))
    return hits


@pytest.mark.parametrize("plant", G.WGRAD_PLANTS)
def test_wgrad_plant_is_rejected(plant):
    hits = _wgrad_hits(plant)
    assert hits, plant
    if plant == "dropped_token_block":
        assert len(hits) == 2 * len(SMALL_WGRAD)
        # the exact form shows a dropped block in every case; random operands of the long cases hide single elements of
        # it inside (T + 2) u S, never all of them
        assert all(v[0] and v[1] for k, v in hits.items() if k.endswith("/exact")), hits
        assert all(v[0] for v in hits.values()), hits
    elif plant == "tail_rows_counted":
        assert len(hits) == 2 * len(SMALL_WGRAD) and all(v[0] and v[1] for v in hits.values()), hits
    elif plant == "dw_transposed":
        assert {k.split("/")[0] for k in hits} == {c.name for c in SMALL_WGRAD if c.N == c.K}
        assert all(v[0] and not v[1] for v in hits.values()), hits
    elif plant == "db_from_last_split_only":
        assert {k.split("/")[0] for k in hits} == {c.name for c in SMALL_WGRAD if G.wgrad_split(*c[1:]).splits > 1}
        assert all(v[1] and not v[0] for v in hits.values()), hits


def _lnb_hits(plant):
    hits = {}
    for c in G.LNB_CASES:
        for first in G.lnb_firsts(c):
            x, dy, gamma = G.make_lnb_inputs(c, first)
            ref = G.ref_layernorm_bwd(x, dy, gamma, G.EPS, c.dx_bf16)
            bad = G.ref_layernorm_bwd(x, dy, gamma, G.EPS, c.dx_bf16, plant=plant)
            got_dx = G.bf16_rn(bad.dx) if c.dx_bf16 else bad.dx
            hits["%s/%d" % (c.name, first)] = (_rejected(lambda: G.check(got_dx, ref.dx, ref.bound_dx)),
                                               _rejected(lambda: G.check(bad.dgamma, ref.dgamma, ref.bound_dgamma)))
    return hits


@pytest.mark.parametrize("plant", G.LNB_PLANTS)
def test_layernorm_bwd_plant_is_rejected(plant):
    hits = _lnb_hits(plant)
    many = {k: v for k, v in hits.items() if not k.startswith("rows1_")}
    if plant == "ln_dgamma_without_xhat":
        assert all(v[1] and not v[0] for v in many.values()), hits
        # one constant row: xhat = 0 and dgamma = 0, the plant gives sum g
        assert all(v[1] for v in hits.values()), hits
    else:
        assert all(v[0] and not v[1] for v in many.values()), hits
        # a single constant row has xhat = 0: the missing term is zero there; every other kind shows it
        shown = [k for k, v in hits.items() if k.startswith("rows1_") and v[0]]
        assert len(shown) >= 3 * 8, (plant, shown)


def test_unknown_plant_is_an_error():
    c = G.WGRAD_CASES[0]
    with pytest.raises(ValueError):
        G.ref_wgrad(c, *G.make_wgrad_inputs(c, False), False, plant="ln_dgamma_without_xhat")
    with pytest.raises(ValueError):
        G.ref_layernorm_bwd(torch.zeros(1, 256), torch.zeros(1, 256), torch.ones(256), G.EPS, False, plant="dw_transposed")
