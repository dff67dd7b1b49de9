"""fp64 references, DERIVED error bounds, cases and planted errors for the training gradients of the BEV transformer's
linears and LayerNorms (tests/test_transformer_grad_gpu.py on the GPU, tests/test_transformer_grad_ref_cpu.py for this
helper itself):

  weight / bias gradient   linear_wgrad_kernel      ops.linear_wgrad     ref_wgrad
  LayerNorm backward       layernorm_bwd_kernel     ops.layernorm_bwd    ref_layernorm_bwd

Everything is fp64 on the CPU, u = 2^-24 as in transformer_gemm_ref, whose conventions (rounding points, `check`,
`NotExercised`, planted errors) hold here too.  No bound is measured on a kernel.

Weight gradient.  dw[n, k] = sum_t dy[t, n] x[t, k], db[n] = sum_t dy[t, n], bf16 operands widened exactly.  A bf16 x
bf16 product is exact in fp32, so dw is a fp32 sum of T exact terms.  The kernel adds them in a tree that the shape
fixes - MFMA blocks of 32 tokens, four waves, the splits' partial tiles, the split-order reduction - and any tree of T
terms satisfies
    |got - ref| <= (T + 2) u sum_t |dy x|            db likewise with sum_t |dy|.
EXACT cases: x from multiples of 1/4 in [-2, 2], dy from multiples of 1/64 in [-1/8, 1/8], T < 2^18.  Every product is
a multiple of 1/256 and every partial sum is below 2^18 / 4 = 2^16: all of them are exact in fp32 in any order
(`_assert_exact_wgrad`), the bound is ZERO and dw, db must equal the fp64 result bit for bit.  That is what catches a
dropped, doubled or misplaced token block, which random operands would hide inside (T + 2) u S.

The split rule of csrc/linear_grad.hip is restated in `wgrad_split` (the CPU ABI test holds it against the library's
workspace size): stages = ceil(T / 128), tiles = (N / 64)(K / 64), want = clamp(512 / tiles, 1, stages),
per = ceil(stages / want), splits = ceil(stages / per); split s owns tokens [128 per s, 128 per (s + 1)).

LayerNorm backward (C = 256).  r = the input row (fp32 or bf16, exact in the kernel), g = the incoming gradient row
(exact), gamma fp32.  With m, d, sigma, xhat = d / sigma of the forward,
    a = g gamma,   m1 = mean a,   m2 = mean(a xhat),   dx = (a - m1 - xhat m2) / sigma,
    dgamma = sum_rows g xhat,   dbeta = sum_rows g.
The kernel (csrc/transformer_pointwise.hip) recomputes mean, d and inv = 1 / sigma' by the forward's two-pass formula
(it never rounds the mean, the forward kernel does: one rounding fewer); transformer_gemm_ref documents the forward's
errors, which bound these too (with E = 0):  dm = (C + 1) u mean|r|,  dd_i = dm + u (|d_i| + dm),
dsigma = rms(dd) + (C / 2 + 4) u sigma,
|d'_i / sigma' - xhat_i| <= e_i = (dd_i + |xhat_i| dsigma) / (sigma - dsigma).  From there, counting operations:
    xhat'   one multiply d' inv':                                 ex_i = e_i + u (|xhat_i| + e_i)
    inv'    |inv' - 1 / sigma| <= dinv = dsigma / (sigma (sigma - dsigma))
    a'      one multiply of exact operands:                       ea_i = u |a_i|
    m1'     a C-term sum in any tree, 1 / C a power of two:       em1 = mean(ea) + (C + 1) u mean(|a| + ea)
    m2'     products a' xhat' (error ep_i = ea_i (|xhat_i| + ex_i) + |a_i| ex_i before their own rounding), rounded or
            fused, then a C-term sum:                              em2 = mean(ep) + (C + 1) u mean(|a xhat| + ep)
    t1      a' - m1':                                             et1 = ea_i + em1 + u (|a_i - m1| + ea_i + em1)
    q       xhat' m2', rounded or fused:  eq0 = ex_i (|m2| + em2) + |xhat_i| em2,   eq = eq0 + u (|xhat_i m2| + eq0)
    t2      t1 - q:                                               et2 = et1 + eq + u (|t2| + et1 + eq)
    dx      t2' inv':       E = et2 (1 / sigma + dinv) + |t2| dinv,   E_dx = E + u (|dx| + E)
    dgamma  R products g xhat' (error |g| ex each, rounded or fused) and an R-term sum in any tree (rows of a wave, the
            four waves, the groups' partials):       E_dgamma = sum |g| ex + (R + 2) u sum (|g xhat| + |g| ex)
    dbeta   E_dbeta = (R + 2) u sum |g|
Every line keeps the first-order terms; what is dropped are products of two of them, each at most (C + 2) u = 1.6e-5
relative, i.e. below 1e-4 of the bound: the bounds are multiplied by SECOND_ORDER = 1.001.  A bf16 dx is one more
round-to-nearest (`bf16_out_bound`).  A constant row (d = 0 exactly, as in the forward's cases) has xhat = 0:
dx = (a - mean a) / sigma there, and the row adds nothing to dgamma.

Planted errors (`plant=`): a deliberately wrong copy of the reference; `NotExercised` where a case cannot show it.
"""
import collections
import functools

import torch

from transformer_gemm_ref import (C, EPS, NotExercised, TINY, U32, _gen, _grid, bf16_out_bound, bf16_rn, check,  # noqa: F401
                                  errors, make_ln_params)

SECOND_ORDER = 1.001
PAD_VALUE = 1e4                 # what the GPU test writes behind x and dy

WGRAD_PLANTS = ("dropped_token_block", "tail_rows_counted", "dw_transposed", "db_from_last_split_only")
LNB_PLANTS = ("ln_bwd_missing_xhat_term", "ln_bwd_gamma_after_mean", "ln_dgamma_without_xhat")

# ----------------------------------------------------------------------------------------------------------------------
# weight gradient
# ----------------------------------------------------------------------------------------------------------------------
WG_TOK, WG_MAXWG = 128, 512
WgradSplit = collections.namedtuple("WgradSplit", "stages per splits")


def wgrad_ok(T, N, K):
    return 1 <= T <= 2 ** 22 and N % 64 == 0 and K % 64 == 0 and 64 <= N <= 1024 and 64 <= K <= 1024


def wgrad_split(T, N, K):
    """The documented split rule of lss_linear_wgrad."""
    stages = -(-T // WG_TOK)
    tiles = (N // 64) * (K // 64)
    want = max(1, min(stages, WG_MAXWG // tiles))
    per = -(-stages // want)
    return WgradSplit(stages, per, -(-stages // per))


def wgrad_workspace_bytes(T, N, K):
    return wgrad_split(T, N, K).splits * (N * K + N) * 4 if wgrad_ok(T, N, K) else 0


WgradCase = collections.namedtuple("WgradCase", "name T N K")
WGRAD_CASES = [
    WgradCase("all_tail", 1, 64, 64),
    WgradCase("one_past_a_block", 33, 64, 64),
    WgradCase("offsets_logits", 4551, 192, 256),        # 3 * 37 * 41 tokens
    WgradCase("value_output_proj", 4551, 256, 256),
    WgradCase("linear1", 1250, 1024, 256),
    WgradCase("linear2", 1250, 256, 1024),
    WgradCase("sample_200x200", 40000, 256, 256),
    # by the split rule: 64 x 64 is one tile, so every 128-token stage is a split of its own: 300 tokens are three
    # splits, the last one of 44 tokens
    WgradCase("three_splits_ragged", 300, 64, 64),
]
WGRAD_BY_NAME = {c.name: c for c in WGRAD_CASES}


def make_wgrad_inputs(c, exact):
    """x (T, K) bf16, dy (T, N) bf16."""
    g = _gen(c.name + ("_exact" if exact else ""))
    if exact:
        return _grid((c.T, c.K), g, 0.25, 2.0).bfloat16(), _grid((c.T, c.N), g, 1.0 / 64, 0.125).bfloat16()
    return torch.randn(c.T, c.K, generator=g).bfloat16(), (0.25 * torch.randn(c.T, c.N, generator=g)).bfloat16()


def _assert_exact_wgrad(x, dy):
    """The operands lie on the grids that make every product and partial sum of dy^T x exact in fp32."""
    for t, q, lim in ((x, 4.0, 2.0), (dy, 64.0, 0.125)):
        assert bool((t * q == torch.round(t * q)).all()) and float(t.abs().max()) <= lim
    assert x.shape[0] < 2 ** 18                      # |partial sum| * 256 <= T * 64 < 2^24


Wgrad = collections.namedtuple("Wgrad", "dw db bound_dw bound_db")


def ref_wgrad(c, x, dy, exact, plant=None):
    """dw (N, K), db (N) in fp64 and the bounds of the kernel's fp32 outputs (zero for the exact cases)."""
    if plant is not None and plant not in WGRAD_PLANTS:
        raise ValueError(plant)
    x, dy = x.double(), dy.double()
    T = x.shape[0]
    assert (T, c.K) == tuple(x.shape) and (T, c.N) == tuple(dy.shape)
    if exact:
        _assert_exact_wgrad(x, dy)
        bound_dw = torch.zeros(c.N, c.K, dtype=torch.float64)
        bound_db = torch.zeros(c.N, dtype=torch.float64)
    else:
        bound_dw = (T + 2) * U32 * (dy.abs().t() @ x.abs()) + TINY
        bound_db = (T + 2) * U32 * dy.abs().sum(0) + TINY
    xs, dys, dyb = x, dy, dy
    if plant == "dropped_token_block":       # the middle 32-token MFMA block
        b = (-(-T // 32)) // 2
        dys = dy.clone()
        dys[32 * b:32 * b + 32] = 0.0
        dyb = dys
    if plant == "db_from_last_split_only":
        sp = wgrad_split(T, c.N, c.K)
        if sp.splits == 1:
            raise NotExercised("one split")
        dyb = dy[WG_TOK * sp.per * (sp.splits - 1):]
    dw, db = dys.t() @ xs, dyb.sum(0)
    if plant == "tail_rows_counted":         # the rows that fill the last 128-token stage, read from behind the tensors
        pad = -T % WG_TOK
        if pad == 0:
            raise NotExercised("no partial stage")
        dw = dw + pad * PAD_VALUE * PAD_VALUE
        db = db + pad * PAD_VALUE
    if plant == "dw_transposed":
        if c.N != c.K:
            raise NotExercised("not square")
        dw = dw.t().contiguous()
    return Wgrad(dw, db, bound_dw, bound_db)


@functools.lru_cache(maxsize=None)
def wgrad_case_data(name, exact):
    """(x, dy, reference) of a case: computed once, shared by the tests that need it, never modified."""
    c = WGRAD_BY_NAME[name]
    x, dy = make_wgrad_inputs(c, exact)
    return x, dy, ref_wgrad(c, x, dy, exact)


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ----------------------------------------------------------------------------------------------------------------------
LN_MAXGROUPS = 1024


def ln_bwd_groups(rows):
    """Row ranges of lss_layernorm_bwd: groups = min(ceil(rows / 4), 1024), rows per group = ceil(rows / groups)."""
    want = min(-(-rows // 4), LN_MAXGROUPS)
    rpg = -(-rows // want)
    return -(-rows // rpg)


LnbCase = collections.namedtuple("LnbCase", "name rows x_bf16 dy_bf16 dx_bf16")
LNB_ROWS = (1, 5, 257, 4551)
_T = lambda b: "bf16" if b else "f32"  # noqa: E731
LNB_CASES = [LnbCase("rows%d_x%s_dy%s_dx%s" % (n, _T(a), _T(b), _T(o)), n, a, b, o)
             for n in LNB_ROWS for a in (False, True) for b in (False, True) for o in (False, True)]
LNB_KINDS = ("unit", "constant", "offset_1000", "tiny_std")


def lnb_firsts(c):
    """Row i of a call is of kind LNB_KINDS[(i + first) % 4]: one call shows every kind from 4 rows on, a shorter case
    takes one call per kind."""
    return (0,) if c.rows >= 4 else (0, 1, 2, 3)


def make_lnb_inputs(c, first=0):
    """x, dy (rows, 256) in the case's dtypes, gamma (256) fp32."""
    g = _gen("lnb_%d_%d" % (c.rows, first))
    z = torch.randn(c.rows, C, generator=g)
    kind = (torch.arange(c.rows) + first) % 4
    const = ((torch.arange(c.rows) % 7).float() * 1.25 - 3.25).view(-1, 1).expand(c.rows, C)  # bf16 values, 3 c exact
    x = torch.where((kind == 0).view(-1, 1), z, torch.zeros(()))
    x = torch.where((kind == 1).view(-1, 1), const, x)
    x = torch.where((kind == 2).view(-1, 1), 1000.0 + z, x)
    x = torch.where((kind == 3).view(-1, 1), 1e-4 * z, x).contiguous()
    dy = torch.randn(c.rows, C, generator=g)
    gamma, _ = make_ln_params(g)
    return (x.bfloat16() if c.x_bf16 else x), (dy.bfloat16() if c.dy_bf16 else dy), gamma


LnBwd = collections.namedtuple("LnBwd", "dx dgamma dbeta bound_dx bound_dgamma bound_dbeta")


def ref_layernorm_bwd(x, dy, gamma, eps, dx_bf16, plant=None):
    """x, dy (rows, 256): the kernel's inputs (any float dtype, widened exactly); returns dx (unrounded), dgamma, dbeta in
    fp64 and the bounds of the kernel's outputs."""
    if plant is not None and plant not in LNB_PLANTS:
        raise ValueError(plant)
    r, g, gm = x.double(), dy.double(), gamma.double()
    R = r.shape[0]
    u = U32
    mean = lambda t: t.mean(-1, keepdim=True)  # noqa: E731
    m = mean(r)
    d = r - m
    sigma = torch.sqrt(mean(d * d) + eps)
    xh = d / sigma
    a = g * gm
    m1, m2 = mean(a), mean(a * xh)
    t2 = a - m1 - xh * m2
    dx = t2 / sigma
    dgamma, dbeta = (g * xh).sum(0), g.sum(0)
    # the forward's errors (transformer_gemm_ref, E = 0)
    dm = (C + 1) * u * mean(r.abs())
    dd = dm + u * (d.abs() + dm)
    ds = torch.sqrt(mean(dd * dd)) + (C / 2 + 4) * u * sigma
    assert bool((ds < sigma).all())
    e = (dd + xh.abs() * ds) / (sigma - ds)
    # the backward's
    ex = e + u * (xh.abs() + e)
    dinv = ds / (sigma * (sigma - ds))
    ea = u * a.abs()
    em1 = mean(ea) + (C + 1) * u * mean(a.abs() + ea)
    ep = ea * (xh.abs() + ex) + a.abs() * ex
    em2 = mean(ep) + (C + 1) * u * mean((a * xh).abs() + ep)
    et1 = ea + em1 + u * ((a - m1).abs() + ea + em1)
    eq0 = ex * (m2.abs() + em2) + xh.abs() * em2
    eq = eq0 + u * ((xh * m2).abs() + eq0)
    et2 = et1 + eq + u * (t2.abs() + et1 + eq)
    E = et2 * (1.0 / sigma + dinv) + t2.abs() * dinv
    E = SECOND_ORDER * (E + u * (dx.abs() + E)) + TINY
    E_dg = SECOND_ORDER * ((g.abs() * ex).sum(0) + (R + 2) * u * ((g * xh).abs() + g.abs() * ex).sum(0)) + TINY
    E_db = SECOND_ORDER * (R + 2) * u * g.abs().sum(0) + TINY
    if plant == "ln_bwd_missing_xhat_term":
        dx = (a - m1) / sigma
    elif plant == "ln_bwd_gamma_after_mean":
        dx = gm * (g - mean(g) - xh * mean(g * xh)) / sigma
    elif plant == "ln_dgamma_without_xhat":
        dgamma = dbeta.clone()
    return LnBwd(dx, dgamma, dbeta, bf16_out_bound(dx, E) if dx_bf16 else E, E_dg, E_db)


def ln_bwd_f32(x, dy, gamma, eps):
    """float32 emulation of layernorm_bwd_kernel's order (sums in torch's tree instead of the wave's)."""
    v, g, gm = x.float(), dy.float(), gamma.float()
    mean = v.sum(-1, keepdim=True) * (1.0 / C)
    d = v - mean
    inv = torch.rsqrt((d * d).sum(-1, keepdim=True) * (1.0 / C) + eps)
    xh = d * inv
    a = g * gm
    m1 = a.sum(-1, keepdim=True) * (1.0 / C)
    m2 = (a * xh).sum(-1, keepdim=True) * (1.0 / C)
    return (a - m1 - xh * m2) * inv, (g * xh).sum(0), g.sum(0)
