"""fp64 references, DERIVED error bounds, cases and planted errors for the tests of the BEV transformer's arithmetic
around the deformable-attention core (tests/test_transformer_gemm_gpu.py on the GPU, tests/test_transformer_gemm_ref_cpu.py
for this helper itself):

  GEMM        linear_mfma_kernel       ops.conv2d_nhwc(1x1, stats=None)   ref_gemm
  FFN         ffn_fused_kernel<false>  ops.ffn_fused                      ref_ffn
  projection  ffn_fused_kernel<true>   ops.linear_res_ln                  ref_linear_res
  LayerNorm   layernorm_kernel         ops.layernorm                      ref_layernorm   (and both fused tails)

Everything is fp64 on the CPU.  u = 2^-24 is the unit roundoff of fp32.  No bound is measured on a kernel.

Rounding points.  Activations and weights enter at their bf16 values, widened exactly (the cases hand the kernels bf16
tensors; nothing is rounded on the way in).  Biases, scale, shift, gamma and beta are fp32 and are never rounded.  A
bf16 OUTPUT is one round-to-nearest of a value v' that carries the pre-rounding error E, |v' - ref| <= E:
    |got - ref| <= E + h(|ref| + E),      h(a) = 2^(floor(log2 a) - 8) = half a bf16 ulp at magnitude a.
bf16 has 8 significant bits, so h(a) lies in (2^-9 a, 2^-8 a]: 2^-9 a is the value of h just below a power of two and
is not a bound anywhere else (1 + 2^-8 rounds to 1: an error of 2^-8).  The exact half ulp is the tightest true bound
and is what `bf16_out_bound` uses.

Dot products.  Any fp32 evaluation of a K-term sum of exact products - any order, any tree, the MFMA's - satisfies
|got - ref| <= (K + 2) u S with S = sum |x w| (+ |b| where a bias is part of the chain), as in depth_head_ref.  (A
bf16 x bf16 product has 16 significant bits: exact in fp32.)  The GEMM epilogue is evaluated in the kernel's order,
    act(scale * acc + shift + residual):
    E_pre = |scale| E_acc + 2 u (|scale| (|acc| + E_acc) + |shift|)        multiply and add, with or without FMA
    E_t   = E_pre + u (|pre| + E_pre + |residual|)                         the residual add
    ReLU is 1-Lipschitz (E unchanged), GELU at most 1.13-Lipschitz: E_out = 1.13 E_t + gelu_bound.

GELU.  Both kernels evaluate 0.5 v (1 + erf(v / sqrt 2)) with erf by Abramowitz & Stegun 7.1.26,
    erf(x) = 1 - Q(t) exp(-x^2),  Q(t) = a1 t + .. + a5 t^5,  t = 1 / (1 + p x),  |formula error| <= 1.5e-7,
as  t = v_rcp_f32(fma(p, |x|, 1));  four FMAs of Horner;  y = 1 - p t __expf(-x x).  Counting operations, with
A(t) = sum |a_i| t^i and B(t) = sum i |a_i| t^i >= |t Q'(t)|:
    t      relative 4u: the rounded constant p (u, since p|x| / (1 + p|x|) < 1), the FMA (u), v_rcp_f32 at 1 ulp (2u);
           it moves Q by at most 4u B(t).
    Q      every term a_i t^i passes through at most four FMAs, the rounding of its constant and the multiply by t:
           at most 6u A(t).
    exp    the argument -x x is rounded (u x^2), scaled by the rounded log2(e) (2u x^2 more) and v_exp_f32 is good to
           1 ulp (2u): relative (3 x^2 + 2) u; one more u for the multiply Q exp.
    1 - .  the result lies in [0, 1]: at most u.
    E_erf(x) = 1.5e-7 + u + u exp(-x^2) (6 A(t) + 4 B(t)) + u q (3 x^2 + 3),   q = erfc|x| + 1.5e-7 >= Q exp(-x^2).
At x = 0 this is 1.5e-7 + 96u = 5.9e-6 (the Horner terms cancel far better than their absolute sum says), at |x| = 1.5
it is 6u and beyond |x| = 3 it is 1.5e-7 + u = 2.1e-7, where it decides whether a hidden unit can round either way.
Around it: x = v * fl(1/sqrt 2) carries 2u |x| and erf' = 2/sqrt(pi) exp(-x^2), the sum 1 + erf is rounded (u, it is
below 2), and 0.5 v (.) is two multiplies:
    |gelu_kernel(v) - gelu(v)| <= 0.5 |v| (E_erf(x) + 2u |x| 2/sqrt(pi) exp(-x^2) + u) + 2u |gelu(v)|.
The CPU test sweeps a float32 emulation of fast_erf and of the whole GELU over 2 * 10^6 points of [-12, 12] and finds
them inside (observed on the emulation: 5.0e-7 at worst - an observation to compare the derivation with, not the
bound).  The direct kernel's libm erff has to sit inside the same bound: E_erf >= 1.5e-7 + u = 3.5 ulp of an erf in
[1/2, 1), more below that; a correctly working erff is good to fewer ulp than that (an assumption about libm that the
GPU test checks, not a derivation).

The fused FFN's bf16 hidden tile never leaves LDS and is rounded in the middle.  Over random operands the dot-product
bound of the pre-activation is about 15 % of half a bf16 ulp, which leaves nearly half of the hidden units free to round
either way: no useful bound follows.  So the FFN cases use EXACT first products: x from multiples of 1/4 in [-2, 2], W1
from multiples of 1/64 in [-1/8, 1/8], b1 from multiples of 1/256 (in [-1, 1]; the lin1_gelu GEMM cases plant +-40 in
four columns).  Every product is a multiple of 1/256 and every partial sum is below 2^16: all of them are exact in fp32
in any order (`_assert_exact`), so the pre-activation v is known exactly and the only uncertainty of a hidden unit is
dh = gelu_bound(v).  A unit is AMBIGUOUS when bf16(h - dh) != bf16(h + dh); an unambiguous unit has one possible value.
    |y - ref| <= (T + 3) u S2 + sum over ambiguous f of |W2[n, f]| (bf16(h + dh) - bf16(h - dh)),
T = the number of nonzero W2[n, :] (zero weights contribute exact zeros: T = F for the dense cases, 1 or 4 for the
identity cases, whose y - x is the sum of one or four hidden units), S2 = sum |h W2| + |b2| + |x|.  Condition, asserted
by the CPU test: at most 5 % of the hidden units of any case are ambiguous.

LayerNorm (row kernel and both fused tails; all three are two-pass).  r_i = the fp64 value of the input row, E_i the
error of the kernel's fp32 copy of it (0 for the row kernel), C = 256, m = mean r, d = r - m, sigma = sqrt(mean d^2 + eps),
yhat = d / sigma:
    mean     fl(sum v) / C in any order: dm = mean(E) + (C + 1) u mean(|r| + E)            (1 / C is a power of two)
    d        dd_i = E_i + dm + u (|d_i| + E_i + dm)
    sigma    a -> sqrt(a^2 + eps) is 1-Lipschitz and the rms is a norm: |rms(d') - rms(d)| <= rms(dd).  The C-term sum of
             squares (one FMA each) is good to (C + 1) u relative, halved by the square root; + eps (u, halved) and
             rsqrtf at 1 ulp (2u): dsigma = rms(dd) + (C / 2 + 4) u sigma            (+ 1 for the second-order terms)
    output   |d' / sigma' - yhat| <= (dd_i + |yhat_i| dsigma) / (sigma - dsigma) = e_i; two multiplies and an add follow:
             E_y = |gamma_i| e_i + 3u (|gamma_i| (|yhat_i| + e_i) + |beta_i|).
A row of 256 equal values whose tripled value is still exact (the cases use bf16 values) sums exactly in any tree:
d = 0 and the output is beta exactly; the GPU test asserts that on top of the bound.

`check` (depth_head_ref) asserts the elementwise bound and returns the two metrics of `train_node_ref.errors`.

Planted errors (`plant=`): a deliberately wrong copy of the reference.  A case that cannot show a plant raises
`NotExercised`; the CPU test proves `check` rejects each plant on at least one committed case.
"""
import collections
import math

import torch

from depth_head_ref import NotExercised, TINY, U32, check  # noqa: F401  (check, NotExercised: re-exported)
from train_node_ref import errors  # noqa: F401

C = 256                      # d_model
EPS = 1e-5
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
AS_ERR = 1.5e-7
GELU_LIP = 1.13
AMBIGUOUS_CAP = 0.05

GEMM_PLANTS = ("dropped_k_step", "residual_after_activation", "shift_before_scale", "bf16_truncated",
               "head_major_pixel_by_tile", "tanh_gelu")
FFN_PLANTS = ("b1_from_previous_chunk", "tanh_gelu", "dropped_hidden_chunk")
LN_PLANTS = ("ln_one_pass_variance", "ln_eps_outside_sqrt", "ln_gamma_beta_swapped")
TAIL_PLANTS = ("tail_rows_from_row_zero",)


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


# ----------------------------------------------------------------------------------------------------------------------
# bf16 in fp64
# ----------------------------------------------------------------------------------------------------------------------
def _exponent(t):
    """frexp exponent e of |t| = m 2^e, 1/2 <= m < 1; bf16's smallest normal binade for 0 and below."""
    e = torch.frexp(t)[1]
    return torch.where(t == 0, torch.full_like(e, -125), e).clamp_min(-125)


def bf16_rn(t):
    """fp64 -> the nearest bf16 value (ties to even), exactly, as fp64: no detour through fp32."""
    ulp = torch.ldexp(torch.ones_like(t), _exponent(t) - 8)
    return torch.round(t / ulp) * ulp


def bf16_trunc(t):
    ulp = torch.ldexp(torch.ones_like(t), _exponent(t) - 8)
    return torch.trunc(t / ulp) * ulp


def bf16_half_ulp(mag):
    """Half a bf16 ulp at magnitude `mag` >= 0."""
    return torch.ldexp(torch.ones_like(mag), _exponent(mag) - 9)


def bf16_out_bound(ref, E):
    return E + bf16_half_ulp(ref.abs() + E)


def f32_out_bound(E):
    return E + TINY


# ----------------------------------------------------------------------------------------------------------------------
# GELU
# ----------------------------------------------------------------------------------------------------------------------
def gelu64(v):
    """0.5 v (1 + erf(v / sqrt 2)) = 0.5 v erfc(-v / sqrt 2): no cancellation in the negative tail."""
    return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))


def tanh_gelu64(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def erf_bound(x):
    """E_erf(x) of the module docstring: formula error plus the fp32 evaluation of fast_erf."""
    ax = x.abs()
    t = 1.0 / (1.0 + AS_P * ax)
    A = sum(abs(a) * t ** (i + 1) for i, a in enumerate(AS_A))
    B = sum((i + 1) * abs(a) * t ** (i + 1) for i, a in enumerate(AS_A))
    q = torch.special.erfc(ax) + AS_ERR
    return AS_ERR + U32 + U32 * torch.exp(-ax * ax) * (6.0 * A + 4.0 * B) + U32 * q * (3.0 * ax * ax + 3.0) + TINY


def gelu_bound(v, ev=0.0):
    """|gelu_kernel(v') - gelu(v')| for |v' - v| <= ev (the Lipschitz term 1.13 ev is the caller's)."""
    x = v / math.sqrt(2.0)
    e = erf_bound(x) + 2.0 * U32 * x.abs() * (2.0 / math.sqrt(math.pi)) * torch.exp(-x * x) + U32
    return 0.5 * (v.abs() + ev) * e + 2.0 * U32 * (gelu64(v).abs() + GELU_LIP * ev)


def _assert_exact(x, w, b):
    """The operands lie on the grids that make every product and partial sum of x . w^T + b exact in fp32."""
    for t, q, lim in ((x, 4.0, 2.0), (w, 64.0, 0.125)):
        assert bool((t * q == torch.round(t * q)).all()) and float(t.abs().max()) <= lim
    assert bool((b * 256.0 == torch.round(b * 256.0)).all())
    S = x.abs() @ w.abs().t() + b.abs()
    assert float(S.max()) * 256.0 < 2.0 ** 24
    v = x @ w.t() + b
    assert bool((v.float().double() == v).all())
    return v


def _grid(shape, g, step, lim):
    n = int(round(lim / step))
    return torch.randint(-n, n + 1, shape, generator=g).double() * step


# ----------------------------------------------------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------------------------------------------------
GemmCase = collections.namedtuple("GemmCase", "name B H W K N scale shift residual act out_f32 head_major exact")
_G = GemmCase
GEMM_CASES = [
    _G("k32_one_row", 1, 1, 1, 32, 64, False, True, False, ACT_NONE, False, False, False),
    _G("k64_ragged_n", 1, 1, 127, 64, 72, True, True, False, ACT_RELU, False, False, False),
    _G("k96_scalar_epilogue", 1, 1, 129, 96, 100, False, True, True, ACT_NONE, True, False, False),
    _G("compress", 2, 10, 10, 128, 256, True, True, False, ACT_RELU, False, False, False),
    _G("offsets_logits", 2, 9, 14, 256, 192, False, True, False, ACT_NONE, True, False, False),
    _G("value_head_major", 3, 5, 10, 256, 256, False, True, False, ACT_NONE, False, True, False),
    _G("lin1_gelu_bf16", 1, 257, 1, 256, 1024, False, True, False, ACT_GELU, False, False, True),
    _G("lin1_gelu_f32", 1, 257, 1, 256, 1024, False, True, False, ACT_GELU, True, False, True),
    _G("lin2", 1, 257, 1, 1024, 256, False, True, True, ACT_NONE, True, False, False),
    _G("grid_9", 1, 300, 1, 64, 384, False, True, False, ACT_NONE, False, False, False),
    _G("grid_12", 1, 389, 1, 64, 320, False, True, True, ACT_NONE, False, False, False),
    # not in the issue's table: the only epilogue with a residual AND an activation (what residual_after_activation needs)
    _G("residual_relu", 1, 1, 130, 64, 128, True, True, True, ACT_RELU, False, False, False),
]
GEMM_BY_NAME = {c.name: c for c in GEMM_CASES}
BIG_B1_COLUMNS = ((3, 40.0), (515, -40.0), (700, 40.0), (1023, -40.0))


def gemm_dispatch_ok(c):
    """The condition under which lss_conv2d_fwd sends a 1x1 / stride-1 bf16 conv without stats to linear_mfma_kernel."""
    return c.K % 32 == 0 and c.N >= 64


def make_gemm_inputs(c):
    """x (B,H,W,K) bf16, w (N,K) bf16, scale / shift (N) fp32 | None, residual (B,H,W,N) bf16 | None."""
    assert gemm_dispatch_ok(c), c.name
    g = _gen("lin1_gelu" if c.exact else c.name)   # the two lin1_gelu cases share their operands
    if c.exact:
        x = _grid((c.B, c.H, c.W, c.K), g, 0.25, 2.0).bfloat16()
        w = _grid((c.N, c.K), g, 1.0 / 64, 0.125).bfloat16()
        shift = _grid((c.N,), g, 1.0 / 256, 1.0).float()
        for col, val in BIG_B1_COLUMNS:
            shift[col] = val
        return dict(x=x, w=w, scale=None, shift=shift, residual=None)
    x = torch.randn(c.B, c.H, c.W, c.K, generator=g).bfloat16()
    w = (torch.randn(c.N, c.K, generator=g) / c.K ** 0.5).bfloat16()
    scale = torch.rand(c.N, generator=g) + 0.5 if c.scale else None
    shift = torch.randn(c.N, generator=g) if c.shift else None
    residual = torch.randn(c.B, c.H, c.W, c.N, generator=g).bfloat16() if c.residual else None
    return dict(x=x, w=w, scale=scale, shift=shift, residual=residual)


def to_head_major(t, B, HW, N):
    """(B*HW, N) rows -> (B, N/32, HW, 32)."""
    return t.reshape(B, HW, N // 32, 32).permute(0, 2, 1, 3).contiguous()


def _head_major_by_tile(t, B, HW, N):
    """The head-major store with the pixel index taken inside the 128-row tile instead of inside the sample."""
    M = B * HW
    out = torch.zeros(B * (N // 32) * HW * 32, dtype=t.dtype)
    rows = t.reshape(M, N // 32, 32)
    for m in range(M):   # ascending m: the last writer wins, as rows of later tiles would
        b, pix = m // HW, m % 128
        for hd in range(N // 32):
            o = ((b * (N // 32) + hd) * HW + pix) * 32
            if o + 32 <= out.numel():
                out[o:o + 32] = rows[m, hd]
    return out.reshape(B, N // 32, HW, 32)


Gemm = collections.namedtuple("Gemm", "out bound pre E_pre S")


def ref_gemm(c, ins, plant=None):
    """out = act(scale * (x . w^T) + shift + residual) UNROUNDED in fp64, shaped as the kernel returns it
    ((B,H,W,N), or (B,N/32,HW,32) with head_major), and the bound of the kernel's (fp32 or bf16) output."""
    if plant is not None and plant not in GEMM_PLANTS:
        raise ValueError(plant)
    M, K, N = c.B * c.H * c.W, c.K, c.N
    x, w = ins["x"].double().reshape(M, K), ins["w"].double()
    sc = None if ins["scale"] is None else ins["scale"].double()
    sh = torch.zeros(N, dtype=torch.float64) if ins["shift"] is None else ins["shift"].double()
    res = None if ins["residual"] is None else ins["residual"].double().reshape(M, N)
    if plant == "shift_before_scale" and (sc is None or ins["shift"] is None):
        raise NotExercised("needs a scale and a shift")
    xs = x
    if plant == "dropped_k_step":   # k-step 1 of the last 32-channel slab: 16-B pieces 1 and 3 of its rows
        xs = x.clone()
        base = K - 32
        xs[:, base + 8:base + 16] = 0.0
        xs[:, base + 24:base + 32] = 0.0
    acc, S = xs @ w.t(), x.abs() @ w.abs().t()
    if c.exact:
        assert sc is None and res is None
        _assert_exact(x, w, sh)
        pre, E = acc + sh, torch.zeros_like(acc)
    else:
        E = (K + 2) * U32 * S
        s1 = torch.ones(N, dtype=torch.float64) if sc is None else sc
        if plant == "shift_before_scale":
            pre = s1 * (acc + sh)
        else:
            pre = s1 * acc + sh
        E = s1.abs() * E + 2.0 * U32 * (s1.abs() * (acc.abs() + E) + sh.abs())
    E_pre, t = E, pre
    late_res = plant == "residual_after_activation"
    if late_res and (res is None or c.act == ACT_NONE):
        raise NotExercised("needs a residual and an activation")
    if res is not None and not late_res:
        t = pre + res
        E = E + U32 * (pre.abs() + E + res.abs())
    if plant == "tanh_gelu" and c.act != ACT_GELU:
        raise NotExercised("no GELU")
    if c.act == ACT_RELU:
        out = torch.relu(t)
    elif c.act == ACT_GELU:
        out = tanh_gelu64(t) if plant == "tanh_gelu" else gelu64(t)
        E = GELU_LIP * E + gelu_bound(t, E)
    else:
        out = t
    if late_res:
        out = out + res
    if plant == "bf16_truncated":
        if c.out_f32:
            raise NotExercised("fp32 output is not rounded")
        out = bf16_trunc(out)
    bound = f32_out_bound(E) if c.out_f32 else bf16_out_bound(out, E)
    if plant == "head_major_pixel_by_tile":
        if not c.head_major:
            raise NotExercised("needs a head-major output")
        return Gemm(_head_major_by_tile(out, c.B, c.H * c.W, N), to_head_major(bound, c.B, c.H * c.W, N), pre, E_pre, S)
    if c.head_major:
        hm = lambda a: to_head_major(a, c.B, c.H * c.W, N)  # noqa: E731
        return Gemm(hm(out), hm(bound), pre, E_pre, S)
    shp = (c.B, c.H, c.W, N)
    return Gemm(out.reshape(shp), bound.reshape(shp), pre, E_pre, S)


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def make_ln_params(g):
    """gamma with zeros and negative entries, beta."""
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::7] = 0.0
    gamma[3::11] *= -1.0
    return gamma, torch.randn(C, generator=g)


def ref_layernorm(r, E, gamma, beta, eps, out_bf16, plant=None):
    """r (rows, 256) fp64: the input rows; E: the elementwise error bound of the kernel's fp32 copy of them (a tensor or
    0.0).  Returns (y unrounded fp64, bound of the kernel's fp32 or bf16 output)."""
    if plant is not None and plant not in LN_PLANTS:
        raise ValueError(plant)
    r = r.double()
    E = torch.zeros_like(r) if not torch.is_tensor(E) else E
    gm, bt = gamma.double(), beta.double()
    m = r.mean(-1, keepdim=True)
    d = r - m
    var = (d * d).mean(-1, keepdim=True)
    sigma = torch.sqrt(var + eps)
    yhat = d / sigma
    y = yhat * gm + bt
    # the bound
    dm = E.mean(-1, keepdim=True) + (C + 1) * U32 * (r.abs() + E).mean(-1, keepdim=True)
    dd = E + dm + U32 * (d.abs() + E + dm)
    ds = torch.sqrt((dd * dd).mean(-1, keepdim=True)) + (C / 2 + 4) * U32 * sigma
    assert bool((ds < sigma).all())
    e = (dd + yhat.abs() * ds) / (sigma - ds)
    Ey = gm.abs() * e + 3.0 * U32 * (gm.abs() * (yhat.abs() + e) + bt.abs())
    if plant == "ln_one_pass_variance":   # fp32 E[x^2] - E[x]^2
        ratio = torch.where(var > 0, m * m / var.clamp_min(1e-300), torch.zeros_like(var))
        if float(ratio.max()) < 5e5:   # fp32 loses u mean^2 of E[x^2]: visible beside the bound from a ratio of about 1e5
            raise NotExercised("no row whose mean dwarfs its spread")
        if bool((bf16_rn(r) == r).all()):   # bf16 rows near 1000 are multiples of 4: their squares sum exactly in fp32
            raise NotExercised("bf16 rows: the fp32 sum of squares is exact")
        r32 = r.float()
        m32 = r32.mean(-1, keepdim=True)
        v32 = ((r32 * r32).mean(-1, keepdim=True) - m32 * m32).clamp_min(0.0)
        y = ((r32 - m32) * torch.rsqrt(v32 + eps)).double() * gm + bt
    elif plant == "ln_eps_outside_sqrt":
        if not bool(((var > 0) & (var <= 1e-2)).any()):
            raise NotExercised("no row whose variance is comparable with eps")
        y = d / (torch.sqrt(var) + eps) * gm + bt
    elif plant == "ln_gamma_beta_swapped":
        y = yhat * bt + gm
    return y, (bf16_out_bound(y, Ey) if out_bf16 else f32_out_bound(Ey))


LnCase = collections.namedtuple("LnCase", "name rows in_bf16 out_bf16")
LN_ROWS = (1, 3, 4, 5, 257)
LN_CASES = [LnCase("rows%d_%s_to_%s" % (n, "bf16" if i else "f32", "bf16" if o else "f32"), n, i, o)
            for n in LN_ROWS for i in (False, True) for o in (False, True)]
LN_KINDS = ("unit", "offset_1000", "constant", "tiny_std", "huge_1e15")


def make_ln_inputs(c, kind):
    """x (rows, 256) in the case's input dtype, gamma, beta.  One kernel call per kind, each of c.rows rows."""
    g = _gen("ln_%d_%s" % (c.rows, kind))
    z = torch.randn(c.rows, C, generator=g)
    if kind == "unit":
        x = z
    elif kind == "offset_1000":
        x = 1000.0 + z
    elif kind == "constant":   # bf16 values: 3 c is exact, so every summation tree is
        x = ((torch.arange(c.rows) % 7).float() * 1.25 - 3.25).view(-1, 1).expand(c.rows, C).contiguous()
    elif kind == "tiny_std":
        x = 1e-4 * z
    elif kind == "huge_1e15":
        x = 1e15 * z
    else:
        raise ValueError(kind)
    gamma, beta = make_ln_params(g)
    return (x.bfloat16() if c.in_bf16 else x), gamma, beta


# ----------------------------------------------------------------------------------------------------------------------
# the fused FFN and the fused output projection
# ----------------------------------------------------------------------------------------------------------------------
def _tail_rows_from_row_zero(t, M):
    """The rows of the partial last 128-token tile all take token 0's row."""
    if M % 128 == 0 or M == 1:
        raise NotExercised("no partial tile besides token 0's")
    t = t.clone()
    t[128 * (M // 128):] = t[0]
    return t


FfnCase = collections.namedtuple("FfnCase", "name F M identity")
FFN_CASES = [FfnCase("f%d_m%d" % (F, M), F, M, False)
             for F, M in ((64, 1), (64, 129), (64, 257), (128, 33), (128, 128), (192, 1), (192, 33), (192, 129),
                          (1024, 128), (1024, 257))]
FFN_CASES += [FfnCase("identity_f256_m257", 256, 257, True), FfnCase("identity_f1024_m130", 1024, 130, True)]
FFN_BY_NAME = {c.name: c for c in FFN_CASES}


def make_ffn_inputs(c):
    """x (M,256) bf16, w1 (F,256) bf16, b1 (F), w2 (256,F) bf16, b2 (256), gamma, beta."""
    g = _gen(c.name)
    x = _grid((c.M, C), g, 0.25, 2.0).bfloat16()
    w1 = _grid((c.F, C), g, 1.0 / 64, 0.125).bfloat16()
    b1 = _grid((c.F,), g, 1.0 / 256, 1.0).float()
    if c.identity:
        w2 = torch.eye(C).repeat(1, c.F // C).bfloat16()
        b2 = torch.zeros(C)
    else:
        w2 = (torch.randn(C, c.F, generator=g) / c.F ** 0.5).bfloat16()
        b2 = torch.randn(C, generator=g)
    gamma, beta = make_ln_params(g)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, gamma=gamma, beta=beta)


Ffn = collections.namedtuple("Ffn", "y bound y_ln bound_ln v h dh lo hi ambiguous clean")


def ref_ffn(ins, plant=None, exact=True, round_hidden=True, eps=EPS):
    """y = x + b2 + W2 . bf16(gelu(W1 . x + b1)) in fp64 and LayerNorm(y) (unrounded), with the bounds of the kernel's
    fp32 y and bf16 y_ln.  `clean` (M,256): no ambiguous hidden unit feeds the element.  exact=False / round_hidden=False:
    arbitrary operands and no rounding of the hidden tile (the chain of the CPU test); no bound then."""
    if plant is not None and plant not in FFN_PLANTS + LN_PLANTS + TAIL_PLANTS:
        raise ValueError(plant)
    x, w1, b1 = ins["x"].double(), ins["w1"].double(), ins["b1"].double()
    w2, b2 = ins["w2"].double(), ins["b2"].double()
    M, F = x.shape[0], w1.shape[0]
    if plant == "b1_from_previous_chunk":
        if F < 128:
            raise NotExercised("one chunk")
        b1 = torch.cat([b1[:64], b1[:-64]])
    v = _assert_exact(x, w1, b1) if exact else x @ w1.t() + b1
    h = tanh_gelu64(v) if plant == "tanh_gelu" else gelu64(v)
    if not round_hidden:
        y = x + b2 + h @ w2.t()
        y_ln = ref_layernorm(y, 0.0, ins["gamma"], ins["beta"], eps, True)[0]
        return Ffn(y, None, y_ln, None, v, h, None, None, None, None, None)
    assert exact
    dh = gelu_bound(v)
    lo, hi, hb = bf16_rn(h - dh), bf16_rn(h + dh), bf16_rn(h)
    amb = lo != hi
    if plant == "dropped_hidden_chunk":
        hb = hb.clone()
        hb[:, F - 64:] = 0.0
    y = x + b2 + hb @ w2.t()
    habs = torch.maximum(lo.abs(), hi.abs())
    S2 = habs @ w2.abs().t() + b2.abs() + x.abs()
    terms = (w2 != 0).sum(1).double()
    E = (terms + 3.0) * U32 * S2 + ((hi - lo) * amb) @ w2.abs().t()
    clean = (amb.double() @ (w2 != 0).double().t()) == 0
    ln_plant = plant if plant in LN_PLANTS else None
    y_ln, bound_ln = ref_layernorm(y, E, ins["gamma"], ins["beta"], eps, True, ln_plant)
    if plant in TAIL_PLANTS:
        y, y_ln = _tail_rows_from_row_zero(y, M), _tail_rows_from_row_zero(y_ln, M)
    return Ffn(y, f32_out_bound(E), y_ln, bound_ln, v, h, dh, lo, hi, amb, clean)


ProjCase = collections.namedtuple("ProjCase", "name M exact offset")
PROJ_CASES = [ProjCase("m%d_%s" % (M, "exact" if ex else "randn"), M, ex, 0.0)
              for M in (1, 127, 128, 300) for ex in (True, False)]
PROJ_CASES += [ProjCase("m300_randn_offset50", 300, False, 50.0)]   # the tail normalises rows whose mean dwarfs the spread
PROJ_BY_NAME = {c.name: c for c in PROJ_CASES}


def make_proj_inputs(c):
    """x (M,256) bf16, w (256,256) bf16, bias (256), residual (M,256) bf16, gamma, beta."""
    g = _gen(c.name)
    if c.exact:
        x = _grid((c.M, C), g, 0.25, 2.0).bfloat16()
        w = _grid((C, C), g, 1.0 / 64, 0.125).bfloat16()
    else:
        x = torch.randn(c.M, C, generator=g).bfloat16()
        w = (torch.randn(C, C, generator=g) / 16.0).bfloat16()
    bias = torch.randn(C, generator=g)
    residual = (torch.randn(c.M, C, generator=g) + c.offset).bfloat16()
    gamma, beta = make_ln_params(g)
    return dict(x=x, w=w, bias=bias, residual=residual, gamma=gamma, beta=beta)


Proj = collections.namedtuple("Proj", "y bound y_ln bound_ln")


def ref_linear_res(ins, exact=False, plant=None, eps=EPS):
    """y = x . W^T + bias + residual in fp64 and LayerNorm(y), with the bounds of the kernel's fp32 y and bf16 y_ln.
    exact: the operands lie on the exact-product grids and the bound is the two roundings of + bias + residual."""
    if plant is not None and plant not in LN_PLANTS + TAIL_PLANTS + ("dropped_k_step",):
        raise ValueError(plant)
    x, w, b, res = ins["x"].double(), ins["w"].double(), ins["bias"].double(), ins["residual"].double()
    xs = x
    if plant == "dropped_k_step":   # the last 16 columns of the last 64-column chunk
        xs = x.clone()
        xs[:, C - 16:] = 0.0
    acc = xs @ w.t()
    y = acc + b + res
    S = x.abs() @ w.abs().t() + b.abs() + res.abs()
    if exact:
        _assert_exact(x, w, torch.zeros(C, dtype=torch.float64))
        E = 2.0 * U32 * (acc.abs() + b.abs() + res.abs())
    else:
        E = (C + 3) * U32 * S
    ln_plant = plant if plant in LN_PLANTS else None
    y_ln, bound_ln = ref_layernorm(y, E, ins["gamma"], ins["beta"], eps, True, ln_plant)
    if plant in TAIL_PLANTS:
        y, y_ln = _tail_rows_from_row_zero(y, x.shape[0]), _tail_rows_from_row_zero(y_ln, x.shape[0])
    return Proj(y, f32_out_bound(E), y_ln, bound_ln)


# ----------------------------------------------------------------------------------------------------------------------
# float32 emulation of fast_erf / the kernels' GELU (the CPU sweep)
# ----------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """float32 fma of float32 tensors: the product is exact in fp64, the sum is rounded to fp64 and then to fp32."""
    return (a.double() * b.double() + c.double()).float()


def fast_erf_f32(x, a=AS_A):
    """csrc/linear_mfma.hip / ffn_fused.hip fast_erf on a float32 tensor, operation by operation (v_rcp_f32 and
    v_exp_f32 replaced by correctly rounded results, which is inside their 1 ulp)."""
    f = lambda s: torch.tensor(s, dtype=torch.float32)  # noqa: E731
    ax = x.abs()
    t = (1.0 / _fma32(f(AS_P), ax, f(1.0)).double()).float()
    p = _fma32(f(a[4]), t, f(a[3]))
    p = _fma32(p, t, f(a[2]))
    p = _fma32(p, t, f(a[1]))
    p = _fma32(p, t, f(a[0]))
    arg = (-ax * ax) * f(1.4426950408889634)          # __expf(a) = v_exp_f32(a * log2(e))
    ex = torch.exp2(arg.double()).float()
    y = 1.0 - p * t * ex
    return torch.copysign(y, x)


def gelu_f32(v):
    return 0.5 * v * (1.0 + fast_erf_f32(v * torch.tensor(0.70710678118654752, dtype=torch.float32)))
