"""fp64 references, DERIVED error bounds, cases, the numpy dropout mask and planted errors for the pointwise training
kernels of the BEV transformer (tests/test_transformer_pointwise_gpu.py on the GPU,
tests/test_transformer_pointwise_ref_cpu.py for this helper itself):

  GELU + dropout           gelu_dropout_kernel<., false>    ops.gelu_dropout                ref_gelu_dropout
  its backward             gelu_dropout_kernel<., true>     ops.gelu_dropout_bwd            ref_gelu_dropout_bwd
  add + dropout + LN       add_dropout_ln_fwd_kernel        ops.add_dropout_layernorm       ref_add_dropout_ln
  its backward             layernorm_bwd_kernel (fused)     ops.add_dropout_layernorm_bwd   ref_add_dropout_ln_bwd

Everything is fp64 on the CPU, u = 2^-24, with the conventions of transformer_gemm_ref / transformer_grad_ref
(rounding points, `check`, `NotExercised`).  No bound is measured on a kernel.

The mask (csrc/dropout_philox.h, restated here independently in numpy).  seed = {key, stream}, two unsigned 64-bit
words.  Element e (the linear index in the contiguous tensor) belongs to call q = e >> 3 of Philox4x32-10 with key
(lo32 key, hi32 key) and counter (q, 0, lo32 stream, hi32 stream), multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
0x9E3779B9 / 0xBB67AE85.  w = out[(e & 7) >> 1], piece = (e & 1) ? w >> 16 : w & 0xffff; keep <=> piece >= thr,
thr = round(p 65536), p_eff = thr / 65536, scale = fp32(1 / (1 - p_eff)); m = keep ? scale : 0.  The references take
the fp32 value of scale that the host passes, so m carries no error.

GELU + dropout.  v = the bf16 hidden (exact), ref = gelu(v) m.  The kernel evaluates transformer_gemm_ref's GELU
(|gelu_kernel - gelu| <= gelu_bound(v)), multiplies by m (u) and rounds to bf16:
    |y - ref| <= bf16_out_bound(ref, scale gelu_bound(v) + 2u |ref|).
A dropped element is EXACTLY zero (finite gelu times 0), a kept one with gelu(v) != 0 is not; the GPU test asserts both
on top of the bound.  v = +-3e38: gelu = v or -0; where |ref| is beyond bf16's largest value (p = 0.5: 6e38) the
output is +-inf as torch's is, and `overflow` marks those elements instead of bounding them.

Its backward.  ref = dy m d(v), d = Phi(v) + v phi(v).  With x = v / sqrt 2 the kernel shares one exponential:
    Phi'  = 0.5 (1 + erf'(x')):   |Phi' - Phi| <= E_Phi = 0.5 (E_erf(x) + 2u |x| 2/sqrt(pi) exp(-x^2) + u)
            (erf_bound, the rounded argument x' = fl(v fl(1/sqrt 2)), the rounded sum: gelu_bound's bracket)
    e'    = v_exp_f32(fl(fl(-x'^2) log2 e)):  the argument v^2 / 2 carries the rounding of h^2 - 2 (2u) from the two
            factors x', u from the square, 2u from the scaling by the rounded log2 e: relative 7u, i.e. an absolute
            7u (v^2 / 2) in the exponent = the same relative error of e' to first order, plus the exponential's
            own relative error, CAPPED at EXP_REL = 2^-21.  The cap is a condition, not a measurement (v_exp_f32 is
            documented at 1 ulp = 2^-23): it still lets every planted error be caught (the CPU test).
    term  = fl(e' fl(1 / sqrt(2 pi))): 2u more.   E_vphi = |v| phi(v) (3.5 u v^2 + EXP_REL + 2u) + TINY
    d'    = fma(v, term, Phi'), then (dy m) d': three roundings, 3u |ref|
    |dh - ref| <= bf16_out_bound(ref, |dy m| (E_Phi + E_vphi) + 3u |ref|).
v = +-3e38: v^2 = inf, e' = 0, v 0 = 0: d is 1 or 0 exactly as in fp64 (phi underflows there too) - never NaN.

Add + dropout + LayerNorm.  s = res + a m with one multiply and one add (res, a exact in the kernel):
    |s' - s| <= 2u |a m| + u |s|                       (the product's u, the sum's u, and their cross term)
Everything downstream - y, ds, dgamma, dbeta - is bounded against the fp64 functions evaluated ON THE KERNEL'S OWN s,
read back: `transformer_gemm_ref.ref_layernorm(s', 0, ..)` and `transformer_grad_ref.ref_layernorm_bwd(s', ..)` with
their bounds; the kernels run exactly those kernels' arithmetic on s'.  da = ds m is one more multiply:
    |da' - da| <= E_ds scale + 2u |da|      (and one bf16 rounding where a is bf16).

Keep rate.  The dropped count of n elements is Binomial(n, p_eff) for an ideal generator: sigma = sqrt(n p (1 - p)).
The CPU test holds the reference mask within 5 sigma (it finds |z| <= 1.6 on the committed sizes and seed), the GPU
capture test within 6 sigma.

Planted errors: `emu_*` are float32 emulations of the kernels' arithmetic (sums in torch's tree); their `plant=` makes
the deliberately wrong kernel.  The CPU test proves the bounds accept the emulation and reject every plant.
"""
import collections
import functools
import math

import numpy as np
import torch

from transformer_gemm_ref import (C, EPS, NotExercised, TINY, U32, _fma32, _gen, bf16_out_bound, bf16_rn, check,  # noqa: F401
                                  erf_bound, fast_erf_f32, gelu64, gelu_bound, gelu_f32, make_ln_params, ref_layernorm)
from transformer_grad_ref import LNB_KINDS, PAD_VALUE, ln_bwd_f32, ref_layernorm_bwd  # noqa: F401

EXP_REL = 2.0 ** -21
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
KEY, STREAM = 0x0123456789ABCDEF, 0x0FEDCBA987654321       # the seed of the committed known answers
PLANTS = ("mask_not_applied_in_backward", "scale_dropped", "mask_shifted_one_call", "pieces_swapped",
          "tanh_gelu_derivative", "da_before_xhat_term")

# ----------------------------------------------------------------------------------------------------------------------
# the mask
# ----------------------------------------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1, _LO = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 values or arrays, key: two uint32 values -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) for v in counter]
    k0, k1 = int(key[0]) & _LO, int(key[1]) & _LO
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_LO),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_LO)]
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c


def pieces(n, key=KEY, stream=STREAM, plant=None):
    """The 16-bit piece of each of the elements 0 .. n - 1 (int64 numpy array)."""
    nq = -(-n // 8)
    q = np.arange(nq, dtype=np.uint64) + np.uint64(1 if plant == "mask_shifted_one_call" else 0)
    zero = np.zeros(nq, dtype=np.uint64)
    w = philox4x32_10((q & np.uint64(_LO), zero, zero + np.uint64(stream & _LO), zero + np.uint64(stream >> 32)),
                      (key & _LO, key >> 32))
    lo = [v & np.uint64(0xFFFF) for v in w]
    hi = [v >> np.uint64(16) for v in w]
    if plant == "pieces_swapped":
        lo, hi = hi, lo
    return np.stack([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3]], 1).reshape(-1)[:n].astype(np.int64)


def threshold(p):
    """p -> (thr, p_eff, scale as the fp32 value the host passes)."""
    thr = int(round(p * 65536.0))
    assert 0 <= thr <= 65535
    return thr, thr / 65536.0, float(np.float32(1.0 / (1.0 - thr / 65536.0)))


def keep_mask(shape, p, key=KEY, stream=STREAM, plant=None):
    """Boolean torch tensor: element kept?  (p = 0: everything.)"""
    n = int(np.prod(shape))
    thr = threshold(p)[0]
    return torch.from_numpy(pieces(n, key, stream, plant) >= thr).reshape(shape)


def multiplier(shape, p, key=KEY, stream=STREAM, plant=None):
    """m in {0, scale} as fp64; all ones for p = 0 / no seed."""
    if p == 0:
        return torch.ones(shape, dtype=torch.float64)
    scale = 1.0 if plant == "scale_dropped" else threshold(p)[2]
    return keep_mask(shape, p, key, stream, plant).double() * scale


def seed_tensor(key=KEY, stream=STREAM, device="cpu"):
    """{key, stream} as the int64[2] the kernels read as unsigned."""
    s = lambda v: v - (1 << 64) if v >= (1 << 63) else v  # noqa: E731
    return torch.tensor([s(key), s(stream)], dtype=torch.int64, device=device)


def seed_words(seed):
    """The inverse: (key, stream) unsigned, from an int64[2] tensor."""
    a, b = (int(v) for v in seed.cpu())
    return a % (1 << 64), b % (1 << 64)


# ----------------------------------------------------------------------------------------------------------------------
# GELU + dropout
# ----------------------------------------------------------------------------------------------------------------------
GELU_SHAPES = ((1, 64), (5, 192), (257, 1024), (4551, 64))
SPECIAL_H = (0.0, -0.0, 30.0, -30.0, 3e38, -3e38)
PS = (0.0, 0.1, 0.5)


@functools.lru_cache(maxsize=None)
def make_gelu_inputs(T, F):
    """h, dy (T, F) bf16: h from multiples of 1/16 in [-12, 12] (bf16 values) with the special values planted at the
    front and, where there is room, across a call's 8 elements further in; dy = randn."""
    g = _gen("gelu_dropout_%d_%d" % (T, F))
    h = (torch.randint(-192, 193, (T, F), generator=g).double() / 16.0).bfloat16()
    dy = torch.randn(T, F, generator=g).bfloat16()
    flat = h.view(-1)
    sp = torch.tensor(SPECIAL_H, dtype=torch.float32).bfloat16()
    for start in (0, 37, 1000, 70001):
        if start + len(SPECIAL_H) <= flat.numel():
            flat[start:start + len(SPECIAL_H)] = sp
    return h, dy


def phi64(v):
    return torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def gelu_grad64(v):
    return 0.5 * torch.special.erfc(-v / math.sqrt(2.0)) + v * phi64(v)


def tanh_gelu_grad64(v):
    k = math.sqrt(2.0 / math.pi)
    t = torch.tanh(k * (v + 0.044715 * v ** 3))
    return 0.5 * (1.0 + t) + 0.5 * v * (1.0 - t * t) * k * (1.0 + 3 * 0.044715 * v * v)


GeluOut = collections.namedtuple("GeluOut", "ref bound overflow")


def ref_gelu_dropout(h, m, scale):
    """h bf16 (any shape), m its multiplier (fp64), scale the kept value of m (1.0 without dropout)."""
    v = h.double()
    ref = gelu64(v) * m
    E = scale * gelu_bound(v) + 2.0 * U32 * ref.abs()
    return GeluOut(ref, bf16_out_bound(ref, E), ref.abs() > BF16_MAX)


def ref_gelu_dropout_bwd(h, dy, m):
    v, g = h.double(), dy.double()
    ref = g * m * gelu_grad64(v)
    x = v / math.sqrt(2.0)
    E_Phi = 0.5 * (erf_bound(x) + 2.0 * U32 * x.abs() * (2.0 / math.sqrt(math.pi)) * torch.exp(-x * x) + U32)
    E_vphi = v.abs() * phi64(v) * (3.5 * U32 * v * v + EXP_REL + 2.0 * U32) + TINY
    E_vphi = torch.where(torch.isfinite(E_vphi), E_vphi, torch.full_like(E_vphi, TINY))   # v = +-3e38: phi = 0, v^2 = inf
    E = (g * m).abs() * (E_Phi + E_vphi) + 3.0 * U32 * ref.abs()
    return GeluOut(ref, bf16_out_bound(ref, E), ref.abs() > BF16_MAX)


_F = lambda s: torch.tensor(s, dtype=torch.float32)  # noqa: E731


def emu_gelu_dropout(h, m):
    """float32 emulation of the forward kernel: gelu_f32 (transformer_gemm_ref), one multiply, bf16."""
    return (gelu_f32(h.float()) * m.float()).bfloat16()


def emu_gelu_dropout_bwd(h, dy, m, plant=None):
    """float32 emulation of the backward kernel, operation by operation."""
    v = h.float()
    x = v * _F(0.70710678118654752)
    if plant == "tanh_gelu_derivative":
        d = tanh_gelu_grad64(v.double()).float()
    else:
        erf = fast_erf_f32(x)
        ax = x.abs()
        e = torch.exp2(((-ax * ax) * _F(1.4426950408889634)).double()).float()
        d = _fma32(v, e * _F(0.3989422804014327), 0.5 * (1.0 + erf))
    mm = torch.ones_like(v) if plant == "mask_not_applied_in_backward" else m.float()
    return (dy.float() * mm * d).bfloat16()


# ----------------------------------------------------------------------------------------------------------------------
# add + dropout + LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 5, 257, 4551)
# (res bf16, a bf16, dy bf16): every (res, a) pair of the forward and every (dy, da = a's dtype) pair of the backward
LN_FORMS = ((False, False, False), (False, True, True), (True, False, True), (True, True, False))
LnCase = collections.namedtuple("LnCase", "name rows res_bf16 a_bf16 dy_bf16")
_T = lambda b: "bf16" if b else "f32"  # noqa: E731
LN_CASES = [LnCase("rows%d_res%s_a%s_dy%s" % (n, _T(r), _T(a), _T(d)), n, r, a, d)
            for n in LN_ROWS for (r, a, d) in LN_FORMS]


def ln_firsts(c):
    """As transformer_grad_ref.lnb_firsts: row i is of kind LNB_KINDS[(i + first) % 4]."""
    return (0,) if c.rows >= 4 else (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def make_ln_inputs(c, first=0):
    """res, a, dy (rows, 256) in the case's dtypes, gamma, beta (256) fp32.  The kinds are those of the SUM: a constant
    row has a = 0, a tiny_std row a tiny a."""
    g = _gen("add_dropout_ln_%d_%d" % (c.rows, first))
    z = torch.randn(c.rows, C, generator=g)
    kind = ((torch.arange(c.rows) + first) % 4).view(-1, 1)
    const = ((torch.arange(c.rows) % 7).float() * 1.25 - 3.25).view(-1, 1).expand(c.rows, C)
    res = torch.where(kind == 0, z, torch.zeros(()))
    res = torch.where(kind == 1, const, res)
    res = torch.where(kind == 2, 1000.0 + z, res)
    res = torch.where(kind == 3, 1e-4 * z, res).contiguous()
    a = 0.5 * torch.randn(c.rows, C, generator=g)
    a = torch.where(kind == 1, torch.zeros(()), a)
    a = torch.where(kind == 3, 1e-4 * a, a).contiguous()
    dy = torch.randn(c.rows, C, generator=g)
    gamma, beta = make_ln_params(g)
    cast = lambda t, b: t.bfloat16() if b else t  # noqa: E731
    return cast(res, c.res_bf16), cast(a, c.a_bf16), cast(dy, c.dy_bf16), gamma, beta


def ref_add(res, a, m):
    """s = res + a m in fp64 and the bound of the kernel's fp32 s."""
    am = a.double() * m
    s = res.double() + am
    return s, 2.0 * U32 * am.abs() + U32 * s.abs() + TINY


AddLnBwd = collections.namedtuple("AddLnBwd", "ds da dgamma dbeta bound_ds bound_da bound_dgamma bound_dbeta")


def ref_add_dropout_ln_bwd(s_got, dy, gamma, eps, m, scale, da_bf16):
    """The fp64 backward ON THE KERNEL'S OWN s (fp32, read back) and the bounds of the kernel's outputs."""
    r = ref_layernorm_bwd(s_got, dy, gamma, eps, False)
    da = r.dx * m
    E = r.bound_dx * scale + 2.0 * U32 * da.abs()
    return AddLnBwd(r.dx, da, r.dgamma, r.dbeta, r.bound_dx, bf16_out_bound(da, E) if da_bf16 else E + TINY,
                    r.bound_dgamma, r.bound_dbeta)


def emu_add(res, a, m):
    """float32: one multiply, one add."""
    return res.float() + a.float() * m.float()


def emu_add_dropout_ln_bwd(s32, dy, gamma, eps, m, da_bf16, plant=None):
    """float32 emulation of the backward kernel on the fp32 sum s32 -> ds, da, dgamma, dbeta."""
    ds, dg, db = ln_bwd_f32(s32, dy, gamma, eps)
    base = ds
    if plant == "da_before_xhat_term":
        v, gm = s32.float(), gamma.float()
        d = v - v.mean(-1, keepdim=True)
        inv = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
        ag = dy.float() * gm
        base = (ag - ag.mean(-1, keepdim=True)) * inv
    mm = torch.ones_like(ds) if plant == "mask_not_applied_in_backward" else m.float()
    da = base * mm
    return ds, (da.bfloat16() if da_bf16 else da), dg, db
