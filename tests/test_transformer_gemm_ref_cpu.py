"""tests/transformer_gemm_ref.py on its own, without a GPU: the references are torch's float64 linear / gelu /
layer_norm, chained with the oracle's sampling core they reproduce the reference project's own transformer fixture, a
float32 emulation of each kernel's order sits inside every case's derived bound, every planted error is rejected by
`check`, the exact-product and ambiguity conditions of the FFN cases hold, and the float32 fast_erf sweep stays inside
the derived E_erf."""
import math
import re

import pytest
import torch
from torch.nn import functional as F

import transformer_gemm_ref as R
from oracle import vovnet_oracle as vo

_id = lambda c: c.name  # noqa: E731


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------------------------
# the references are the operations
# ----------------------------------------------------------------------------------------------------------------------
def test_bf16_helpers_are_round_to_nearest_even():
    g = torch.Generator().manual_seed(1)
    z = torch.cat([torch.randn(4000, generator=g) * 10.0 ** torch.randint(-30, 30, (4000,), generator=g),
                   torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 2.0 ** -126])])
    assert torch.equal(R.bf16_rn(z.double()), z.bfloat16().double())
    assert float(R.bf16_rn(torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64))) == 1.0          # the tie goes to even
    assert float(R.bf16_rn(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64))) == 1.0 + 2.0 ** -7
    m = torch.tensor([1.0, 1.99, 2.0, 0.75], dtype=torch.float64)
    assert R.bf16_half_ulp(m).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9]
    # the half ulp is attained: no smaller relative constant is a bound
    v = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)
    assert float((R.bf16_rn(v) - v).abs()) == float(R.bf16_half_ulp(v))
    t = torch.tensor([1.0 + 2.0 ** -7 - 2.0 ** -20, -3.99], dtype=torch.float64)
    assert R.bf16_trunc(t).tolist() == [1.0, -3.984375]


@pytest.mark.parametrize("c", R.GEMM_CASES, ids=_id)
def test_gemm_reference_is_float64_linear(c):
    ins = R.make_gemm_inputs(c)
    ref = R.ref_gemm(c, ins)
    M = c.B * c.H * c.W
    x, w = ins["x"].double().reshape(M, c.K), ins["w"].double()
    acc = F.linear(x, w)
    if ins["scale"] is not None:
        acc = acc * ins["scale"].double()
    if ins["shift"] is not None:
        acc = acc + ins["shift"].double()
    if ins["residual"] is not None:
        acc = acc + ins["residual"].double().reshape(M, c.N)
    want = {R.ACT_NONE: lambda t: t, R.ACT_RELU: F.relu, R.ACT_GELU: F.gelu}[c.act](acc)
    got = ref.out
    if c.head_major:
        assert got.shape == (c.B, c.N // 32, c.H * c.W, 32)
        got = got.permute(0, 2, 1, 3).reshape(M, c.N)
    assert float((got.reshape(M, c.N) - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert ref.bound.shape == ref.out.shape and bool((ref.bound > 0).all())
    assert (ref.out.dtype, ref.bound.dtype) == (torch.float64, torch.float64)


def test_gelu_reference_and_its_negative_tail():
    v = torch.linspace(-9, 9, 20001, dtype=torch.float64)
    assert float((R.gelu64(v) - F.gelu(v)).abs().max()) <= 1e-12
    # 1 + erf cancels in the tail; erfc does not: the reference keeps its relative accuracy where |h| << |v|
    t = torch.tensor([-8.0], dtype=torch.float64)
    assert abs(float(R.gelu64(t)) / (-8.0 * 0.5 * math.erfc(8.0 / math.sqrt(2.0))) - 1.0) < 1e-14
    assert float((R.tanh_gelu64(v) - F.gelu(v, approximate="tanh")).abs().max()) <= 1e-12
    assert 1e-4 < float((R.tanh_gelu64(v) - R.gelu64(v)).abs().max()) < 1e-3
    d = (R.gelu64(v)[1:] - R.gelu64(v)[:-1]) / (v[1:] - v[:-1])
    assert float(d.abs().max()) <= R.GELU_LIP


@pytest.mark.parametrize("c", R.LN_CASES[:4] + R.LN_CASES[-4:], ids=_id)
def test_layernorm_reference_is_float64_layer_norm(c):
    for kind in R.LN_KINDS:
        x, gamma, beta = R.make_ln_inputs(c, kind)
        y, bound = R.ref_layernorm(x.double(), 0.0, gamma, beta, R.EPS, c.out_bf16)
        want = F.layer_norm(x.double(), (R.C,), gamma.double(), beta.double(), R.EPS)
        assert float((y - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        if kind == "constant":
            assert torch.equal(y, beta.double().expand_as(y))


def test_ffn_and_projection_references_are_float64_compositions():
    for c in (R.FFN_BY_NAME["f192_m33"], R.FFN_BY_NAME["identity_f1024_m130"]):
        ins = R.make_ffn_inputs(c)
        d = {k: v.double() for k, v in ins.items()}
        free = R.ref_ffn(ins, exact=False, round_hidden=False)
        hid = F.gelu(F.linear(d["x"], d["w1"], d["b1"]))
        want = d["x"] + F.linear(hid, d["w2"], d["b2"])
        assert float((free.y - want).abs().max()) <= 1e-12
        ln = F.layer_norm(want, (R.C,), d["gamma"], d["beta"], R.EPS)
        assert float((free.y_ln - ln).abs().max()) <= 1e-12
        ref = R.ref_ffn(ins)
        # torch's own rounding, except where a detour through fp32 could round twice: only ambiguous units can
        hb = hid.float().bfloat16().double()
        assert torch.equal(hb[~ref.ambiguous], R.bf16_rn(ref.h)[~ref.ambiguous])
        want = d["x"] + F.linear(torch.where(ref.ambiguous, R.bf16_rn(ref.h), hb), d["w2"], d["b2"])
        assert float((ref.y - want).abs().max()) <= 1e-12
    for c in R.PROJ_CASES:
        ins = R.make_proj_inputs(c)
        d = {k: v.double() for k, v in ins.items()}
        ref = R.ref_linear_res(ins, c.exact)
        want = F.linear(d["x"], d["w"], d["bias"]) + d["residual"]
        assert float((ref.y - want).abs().max()) <= 1e-12 * float(want.abs().max())
        ln = F.layer_norm(want, (R.C,), d["gamma"], d["beta"], R.EPS)
        assert float((ref.y_ln - ln).abs().max()) <= 1e-11


def test_references_chained_with_the_sampling_core_reproduce_the_fixture(golden):
    """value / offsets / weights projections (ref_gemm), the oracle's bilinear sampling core, the output projection with
    its residual and norm1 (ref_linear_res), the FFN and norm2 (ref_ffn), all in float64 with no bf16 rounding anywhere,
    against `out` of g11_bev_transformer.npz, which the reference project's own classes wrote in float32."""
    g = golden("g11_bev_transformer")
    sd = vo.seeded_state(vo.transformer_shapes(), int(g["seed"]))
    a = "encoder.self_attn."
    sd[a + "sampling_offsets.bias"] = sd[a + "sampling_offsets.bias"] * float(g["bias_scale"])
    sd = {k: v.double() for k, v in sd.items()}
    x = torch.from_numpy(g["x"]).double()
    B, Cc, H, W = x.shape
    N, nh, npt, ch = H * W, 8, 8, Cc // 8
    src = x.flatten(2).permute(0, 2, 1)
    q = src + vo.position_embedding_sine(H, W, Cc // 2).double().flatten(1).t()[None]

    def lin(inp, key):
        w, b = sd[a + key + ".weight"], sd[a + key + ".bias"]
        c = R.GemmCase(key, B, N, 1, Cc, w.shape[0], False, True, False, R.ACT_NONE, True, False, False)
        return R.ref_gemm(c, dict(x=inp, w=w, scale=None, shift=b, residual=None)).out.reshape(B, N, w.shape[0])

    off = lin(q, "sampling_offsets").view(B, N, nh, npt, 2)
    aw = torch.softmax(lin(q, "attention_weights").view(B, N, nh, npt), -1)
    v = lin(src, "value_proj").view(B, H, W, nh, ch)
    loc = (vo.reference_points(H, W).double()[None, :, None, None, :] + off / H).clamp(0, 1)
    attn = torch.zeros(B, N, nh, ch, dtype=torch.float64)
    for h in range(nh):
        gg = loc[:, :, h] * 2.0 - 1.0
        px, py = ((gg[..., 0] + 1) * W - 1) / 2, ((gg[..., 1] + 1) * H - 1) / 2
        s = vo.bilinear_zero_pad(v[:, :, :, h], px.reshape(B, -1), py.reshape(B, -1)).view(B, N, npt, ch)
        attn[:, :, h] = (s * aw[:, :, h, :, None]).sum(2)
    e = "encoder."
    proj = R.ref_linear_res(dict(x=attn.reshape(B * N, Cc), w=sd[a + "output_proj.weight"], bias=sd[a + "output_proj.bias"],
                                 residual=src.reshape(B * N, Cc), gamma=sd[e + "norm1.weight"], beta=sd[e + "norm1.bias"]))
    ffn = R.ref_ffn(dict(x=proj.y_ln, w1=sd[e + "linear1.weight"], b1=sd[e + "linear1.bias"], w2=sd[e + "linear2.weight"],
                         b2=sd[e + "linear2.bias"], gamma=sd[e + "norm2.weight"], beta=sd[e + "norm2.bias"]),
                    exact=False, round_hidden=False)
    out = ffn.y_ln.reshape(B, N, Cc).permute(0, 2, 1).reshape(B, Cc, H, W)
    want = torch.from_numpy(g["out"]).double()
    emax, el2 = R.errors(out, want)
    assert emax <= 1e-5 and el2 <= 2e-6, (emax, el2)    # float32 noise of the fixture's own arithmetic


# ----------------------------------------------------------------------------------------------------------------------
# fast_erf in float32 against the derived E_erf
# ----------------------------------------------------------------------------------------------------------------------
def test_fast_erf_float32_sweep_is_inside_the_derived_bound():
    x = torch.linspace(-12.0, 12.0, 2000001, dtype=torch.float64).float()
    x64 = x.double()
    err = (R.fast_erf_f32(x).double() - torch.erf(x64)).abs()
    bound = R.erf_bound(x64)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert 3e-7 < float(err.max()) < float(bound.max())       # the emulation is not the fp64 formula
    far = x64.abs() >= 3.0
    assert float(bound[far].max()) <= R.AS_ERR + 1.2 * R.U32  # where hidden units can round either way: 1.5e-7 + u
    gerr = (R.gelu_f32(x).double() - R.gelu64(x64)).abs()
    gb = R.gelu_bound(x64)
    assert bool((gerr <= gb).all()), float((gerr / gb).max())
    # libm-grade erf (float32 erf of torch) sits inside the same bound: what the direct kernel's erff needs
    lib = (torch.erf(x).double() - torch.erf(x64)).abs()
    assert bool((lib <= bound).all())
    glib = ((0.5 * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752)))).double() - R.gelu64(x64)).abs()
    assert bool((glib <= gb).all())
    # a wrong digit in one coefficient is outside it
    wrong = list(R.AS_A)
    wrong[2] += 1e-5
    werr = (R.fast_erf_f32(x, wrong).double() - torch.erf(x64)).abs()
    assert bool((werr > bound).any())


# ----------------------------------------------------------------------------------------------------------------------
# the exact-product device
# ----------------------------------------------------------------------------------------------------------------------
def test_exact_product_assertion_rejects_operands_off_the_grid():
    ins = R.make_ffn_inputs(R.FFN_BY_NAME["f64_m129"])
    x, w1, b1 = ins["x"].double(), ins["w1"].double(), ins["b1"].double()
    v = R._assert_exact(x, w1, b1)
    assert bool((v == (x.float() @ w1.float().t() + b1.float()).double()).all())     # a float32 matmul is exact too
    for bad in ((x + 1.0 / 8, w1, b1), (x, w1 + 1.0 / 128, b1), (x, w1, b1 + 1.0 / 512), (x * 2.0, w1, b1)):
        with pytest.raises(AssertionError):
            R._assert_exact(*bad)
    with pytest.raises(AssertionError):   # random operands: the products are not on the grid
        R.ref_ffn(dict(ins, x=torch.randn(129, 256).bfloat16()))


@pytest.mark.parametrize("c", R.FFN_CASES, ids=_id)
def test_ffn_case_conditions(c):
    ins = R.make_ffn_inputs(c)
    ref = R.ref_ffn(ins)
    share = float(ref.ambiguous.double().mean())
    print("ambiguous hidden units of %s: %.4f" % (c.name, share))
    assert share <= R.AMBIGUOUS_CAP, share
    assert bool((ref.lo <= ref.hi).all()) and bool((R.bf16_rn(ref.h) >= ref.lo).all())
    assert 1.2 < float(ref.v.std()) < 2.0 and float(ref.v.abs().max()) < 9.0
    assert float(ins["b1"].abs().max()) <= 1.0
    if c.identity:
        assert float(ref.clean.double().mean()) >= 0.9
        d = ins["w2"].double()
        assert bool((d.sum(1) == c.F // R.C).all()) and bool(((d == 0) | (d == 1)).all()) and not ins["b2"].any()
        # every clean element is known to the roundings of its adds alone
        blocks = c.F // R.C
        y_minus_x = R.bf16_rn(ref.h).reshape(c.M, blocks, R.C).sum(1)
        assert torch.equal(ref.y - ins["x"].double(), y_minus_x)
        tight = (blocks + 3) * R.U32 * (R.bf16_rn(ref.h).abs().reshape(c.M, blocks, R.C).sum(1) + ins["x"].double().abs())
        assert bool((ref.bound[ref.clean] <= tight[ref.clean] * (1 + 1e-9) + R.TINY).all())
        bad = R.ref_ffn(ins, plant="tanh_gelu")
        wrong = ((bad.y - ref.y).abs() > ref.bound) & ref.clean
        assert int(wrong.sum()) >= 100, int(wrong.sum())


def test_case_tables_cover_what_they_must():
    by = R.GEMM_BY_NAME
    assert all(R.gemm_dispatch_ok(c) for c in R.GEMM_CASES)
    assert {c.K // 32 for c in R.GEMM_CASES} >= {1, 2, 3, 4, 8, 32}            # the three prologues and the steady state
    assert any(c.N % 8 for c in R.GEMM_CASES) and any(c.N % 128 for c in R.GEMM_CASES if c.N % 8 == 0)
    hm = by["value_head_major"]
    assert hm.head_major and hm.H * hm.W < 128 < hm.B * hm.H * hm.W and 128 % (hm.H * hm.W)   # a tile spans samples
    grids = {c.name: -(-c.B * c.H * c.W // 128) * -(-c.N // 128) for c in R.GEMM_CASES}
    assert grids["grid_9"] == 9 and grids["grid_12"] == 12 and grids["k32_one_row"] == 1
    assert by["k32_one_row"].B * by["k32_one_row"].H * by["k32_one_row"].W == 1
    assert {c.F for c in R.FFN_CASES if not c.identity} == {64, 128, 192, 1024}
    for M in (1, 33, 128, 129, 257):
        assert sum(1 for c in R.FFN_CASES if c.M == M and not c.identity) >= 2
    for Fv in (64, 128, 192, 1024):
        assert sum(1 for c in R.FFN_CASES if c.F == Fv and not c.identity) >= 2
    assert {(c.F, c.M) for c in R.FFN_CASES if c.identity} == {(256, 257), (1024, 130)}
    assert {(c.M, c.exact) for c in R.PROJ_CASES} == {(m, e) for m in (1, 127, 128, 300) for e in (True, False)}
    assert sum(1 for c in R.PROJ_CASES if c.offset) == 1
    assert len(R.LN_CASES) == 20 and {c.rows for c in R.LN_CASES} == {1, 3, 4, 5, 257}
    ins = R.make_gemm_inputs(by["lin1_gelu_bf16"])
    assert sorted(float(ins["shift"][col]) for col, _ in R.BIG_B1_COLUMNS) == [-40.0, -40.0, 40.0, 40.0]
    assert all(torch.equal(ins[k], R.make_gemm_inputs(by["lin1_gelu_f32"])[k]) for k in ("x", "w", "shift"))
    g, _ = R.make_ln_params(torch.Generator().manual_seed(0))
    assert bool((g == 0).any()) and bool((g < 0).any()) and bool((g > 0).any())


# ----------------------------------------------------------------------------------------------------------------------
# a float32 emulation of each kernel's order stays inside the bound
# ----------------------------------------------------------------------------------------------------------------------
def _ln_f32(v, gamma, beta, eps):
    """Two-pass, as the kernels."""
    mean = v.sum(-1, keepdim=True) * (1.0 / R.C)
    d = v - mean
    inv = torch.rsqrt((d * d).sum(-1, keepdim=True) * (1.0 / R.C) + eps)
    return d * inv * gamma + beta


@pytest.mark.parametrize("c", R.GEMM_CASES, ids=_id)
def test_gemm_float32_emulation_is_inside_the_bound(c):
    ins = R.make_gemm_inputs(c)
    ref = R.ref_gemm(c, ins)
    M = c.B * c.H * c.W
    acc = ins["x"].float().reshape(M, c.K) @ ins["w"].float().t()
    if ins["scale"] is not None:
        acc = acc * ins["scale"]
    if ins["shift"] is not None:
        acc = acc + ins["shift"]
    if ins["residual"] is not None:
        acc = acc + ins["residual"].float().reshape(M, c.N)
    out = R.gelu_f32(acc) if c.act == R.ACT_GELU else F.relu(acc) if c.act == R.ACT_RELU else acc
    if not c.out_f32:
        out = out.bfloat16()
    out = R.to_head_major(out, c.B, c.H * c.W, c.N) if c.head_major else out.reshape(c.B, c.H, c.W, c.N)
    R.check(out, ref.out, ref.bound, c.name)
    if c.exact:
        assert not ref.E_pre.any()
        big = [col for col, _ in R.BIG_B1_COLUMNS]
        assert float(ref.pre[:, big].abs().min()) > 30.0 and bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("c", R.FFN_CASES, ids=_id)
def test_ffn_float32_emulation_is_inside_the_bound(c):
    ins = R.make_ffn_inputs(c)
    ref = R.ref_ffn(ins)
    x = ins["x"].float()
    hid = R.gelu_f32(x @ ins["w1"].float().t() + ins["b1"]).bfloat16().float()
    y = hid @ ins["w2"].float().t() + ins["b2"] + x
    R.check(y, ref.y, ref.bound, c.name)
    R.check(_ln_f32(y, ins["gamma"], ins["beta"], R.EPS).bfloat16(), ref.y_ln, ref.bound_ln, c.name + ".ln")
    # torch's own float32 GELU (libm erf) rounds the unambiguous units to the same bf16 values
    hid2 = F.gelu(x @ ins["w1"].float().t() + ins["b1"]).bfloat16().float()
    assert torch.equal(hid2[~ref.ambiguous], R.bf16_rn(ref.h).float()[~ref.ambiguous])
    assert torch.equal(hid[~ref.ambiguous], hid2[~ref.ambiguous])


@pytest.mark.parametrize("c", R.PROJ_CASES, ids=_id)
def test_projection_float32_emulation_is_inside_the_bound(c):
    ins = R.make_proj_inputs(c)
    ref = R.ref_linear_res(ins, c.exact)
    y = ins["x"].float() @ ins["w"].float().t() + ins["bias"] + ins["residual"].float()
    R.check(y, ref.y, ref.bound, c.name)
    R.check(_ln_f32(y, ins["gamma"], ins["beta"], R.EPS).bfloat16(), ref.y_ln, ref.bound_ln, c.name + ".ln")
    if c.offset:
        m, s = ref.y.mean(-1), ref.y.std(-1)
        assert float((m.abs() / s).min()) > 20.0
    if c.exact:   # the bound is two roundings wide
        d = {k: v.double() for k, v in ins.items()}
        S = (d["x"] @ d["w"].t()).abs() + d["bias"].abs() + d["residual"].abs()
        assert bool((ref.bound <= 2.0 * R.U32 * S + R.TINY).all())


@pytest.mark.parametrize("c", R.LN_CASES, ids=_id)
def test_layernorm_float32_emulation_is_inside_the_bound(c):
    for kind in R.LN_KINDS:
        x, gamma, beta = R.make_ln_inputs(c, kind)
        y, bound = R.ref_layernorm(x.double(), 0.0, gamma, beta, R.EPS, c.out_bf16)
        got = _ln_f32(x.float(), gamma, beta, R.EPS)
        got = got.bfloat16() if c.out_bf16 else got
        R.check(got, y, bound, "%s.%s" % (c.name, kind))
        if kind == "constant":
            assert torch.equal(got.float(), (beta.bfloat16().float() if c.out_bf16 else beta).expand_as(got))
        if kind == "tiny_std":
            assert float(x.double().var(-1, unbiased=False).max()) < 1e-2 * R.EPS


# ----------------------------------------------------------------------------------------------------------------------
# planted errors
# ----------------------------------------------------------------------------------------------------------------------
def _gemm_hits(plant):
    hits = {}
    for c in R.GEMM_CASES:
        ins = R.make_gemm_inputs(c)
        try:
            bad = R.ref_gemm(c, ins, plant=plant)
        except R.NotExercised:
            continue
        ref = R.ref_gemm(c, ins)
        got = bad.out if c.out_f32 else R.bf16_rn(bad.out) if plant != "bf16_truncated" else bad.out
        hits["gemm/" + c.name] = _rejected(lambda: R.check(got, ref.out, ref.bound))
    return hits


def _ffn_hits(plant):
    hits = {}
    for c in R.FFN_CASES:
        ins = R.make_ffn_inputs(c)
        try:
            bad = R.ref_ffn(ins, plant=plant)
        except R.NotExercised:
            continue
        ref = R.ref_ffn(ins)
        if plant not in R.LN_PLANTS:
            hits["ffn/" + c.name] = _rejected(lambda: R.check(bad.y, ref.y, ref.bound))
        hits["ffn_ln/" + c.name] = _rejected(lambda: R.check(R.bf16_rn(bad.y_ln), ref.y_ln, ref.bound_ln))
    return hits


def _proj_hits(plant):
    hits = {}
    for c in R.PROJ_CASES:
        ins = R.make_proj_inputs(c)
        try:
            bad = R.ref_linear_res(ins, c.exact, plant=plant)
        except R.NotExercised:
            continue
        ref = R.ref_linear_res(ins, c.exact)
        if plant not in R.LN_PLANTS:
            hits["proj/" + c.name] = _rejected(lambda: R.check(bad.y, ref.y, ref.bound))
        hits["proj_ln/" + c.name] = _rejected(lambda: R.check(R.bf16_rn(bad.y_ln), ref.y_ln, ref.bound_ln))
    return hits


def _ln_hits(plant):
    hits = {}
    for c in R.LN_CASES:
        for kind in R.LN_KINDS:
            x, gamma, beta = R.make_ln_inputs(c, kind)
            try:
                bad, _ = R.ref_layernorm(x.double(), 0.0, gamma, beta, R.EPS, c.out_bf16, plant=plant)
            except R.NotExercised:
                continue
            y, bound = R.ref_layernorm(x.double(), 0.0, gamma, beta, R.EPS, c.out_bf16)
            got = R.bf16_rn(bad) if c.out_bf16 else bad
            hits["ln/%s/%s" % (c.name, kind)] = _rejected(lambda: R.check(got, y, bound))
    return hits


@pytest.mark.parametrize("plant", R.GEMM_PLANTS)
def test_gemm_plant_is_rejected(plant):
    hits = _gemm_hits(plant)
    assert hits and all(hits.values()), (plant, hits)
    names = set(hits)
    if plant == "dropped_k_step":
        assert len(hits) == len(R.GEMM_CASES)
        assert all(_proj_hits(plant).values())
    if plant == "residual_after_activation":
        assert names == {"gemm/residual_relu"}
    if plant == "shift_before_scale":
        assert names == {"gemm/k64_ragged_n", "gemm/compress", "gemm/residual_relu"}
    if plant == "bf16_truncated":
        assert names == {"gemm/" + c.name for c in R.GEMM_CASES if not c.out_f32}
    if plant == "head_major_pixel_by_tile":
        assert names == {"gemm/value_head_major"}
    if plant == "tanh_gelu":
        assert names == {"gemm/lin1_gelu_bf16", "gemm/lin1_gelu_f32"}


@pytest.mark.parametrize("plant", R.FFN_PLANTS)
def test_ffn_plant_is_rejected(plant):
    hits = _ffn_hits(plant)
    assert hits, plant
    if plant == "b1_from_previous_chunk":
        assert not any("/f64_" in k for k in hits)
    # the fp32 output shows every plant on every case that exercises it; behind the LayerNorm and the bf16 rounding a
    # one-token case with three changed hidden units may not
    assert all(v for k, v in hits.items() if k.startswith("ffn/")), (plant, hits)
    assert sum(v for k, v in hits.items() if k.startswith("ffn_ln/")) >= len(hits) // 2 - 2, (plant, hits)


@pytest.mark.parametrize("plant", R.LN_PLANTS)
def test_layernorm_plant_is_rejected(plant):
    hits = _ln_hits(plant)
    assert hits and all(hits.values()), (plant, {k: v for k, v in hits.items() if not v})
    kinds = {k.split("/")[-1] for k in hits}
    if plant == "ln_one_pass_variance":
        assert kinds == {"offset_1000"}
    if plant == "ln_eps_outside_sqrt":
        assert kinds == {"tiny_std"}
    if plant == "ln_gamma_beta_swapped":
        assert kinds == set(R.LN_KINDS) and len(hits) == len(R.LN_CASES) * len(R.LN_KINDS)
        fused = dict(_ffn_hits(plant), **_proj_hits(plant))
        assert fused and all(fused.values()), fused


@pytest.mark.parametrize("plant", R.TAIL_PLANTS)
def test_tail_plant_is_rejected(plant):
    hits = dict(_ffn_hits(plant), **_proj_hits(plant))
    assert hits and all(hits.values()), (plant, hits)
    ms = {int(re.search(r"[/_]m(\d+)", k).group(1)) for k in hits}
    assert ms == {33, 129, 257, 130, 127, 300}     # every partial tile except the one-token cases


def test_unknown_plant_is_an_error():
    c = R.GEMM_CASES[0]
    with pytest.raises(ValueError):
        R.ref_gemm(c, R.make_gemm_inputs(c), plant="no_such_plant")
    with pytest.raises(ValueError):
        R.ref_ffn(R.make_ffn_inputs(R.FFN_CASES[0]), plant="dropped_k_step")
    with pytest.raises(ValueError):
        R.ref_layernorm(torch.zeros(1, 256, dtype=torch.float64), 0.0, torch.ones(256), torch.zeros(256), R.EPS, False,
                        plant="tanh_gelu")
