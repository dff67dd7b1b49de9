"""fp64 reference, DERIVED error bounds, cases and planted errors for K10, the clipped Adam step of csrc/optim.hip
(tests/test_clip_adam_gpu.py on the GPU, tests/test_clip_adam_ref_cpu.py for this helper itself):

  sum of squares    sqnorm_partials_kernel   one partial per 4096-element chunk of one tensor
  finalize          clip_finalize_kernel     norm, clip coefficient, step count, the two bias corrections -> state[0..4]
  update            clip_adam_kernel         g *= coef;  Adam on p, m, v

Conventions of transformer_gemm_ref / transformer_pointwise_ref: everything is fp64 on the CPU, u = 2^-24, `check`
asserts an elementwise bound, a case that cannot show a planted error raises `NotExercised`.  No bound is measured on a
kernel.

The contract.  K10 is torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (amsgrad = False, maximize = False) WITH
FP32-ROUNDED HYPER-PARAMETERS: the host passes lr, beta1, beta2, eps, weight_decay and max_norm as C floats, so the
reference takes float(np.float32(lr)) and so on, and the clip's constant is the kernel's 1e-6f.  `ref_step` is that
update on lists of numpy arrays in fp64; the CPU test holds it to 1e-12 of torch's own float64 run.

The five state floats, against fp64 evaluated on the fp32 gradients (`ref_scalars`).

  Norm.  S = sum g^2 has only non-negative terms, so a term that passes through at most D roundings leaves the sum
  with a relative error of at most gamma_D = D u / (1 - D u).  D is read off the kernels: a thread's chain of 16 fmas
  (4 float4 loads; the first fma rounds too), the 6 levels of `lss_wave_sum`'s xor butterfly (every lane adds the
  same pair, so it is a 6-level tree), the 4-way add (red0 + red1) + (red2 + red3) (2), the finalize's strided chain
  of L = ceil(nb / 256) adds and its 8-level tree over 256 threads: D = 32 + L.  sqrtf is correctly rounded
  (SQRT_REL = u: optim.hip is built without fast-math flags, hipcc's default is the IEEE square root and divide):
      |norm' - norm| <= (a + u + a u) norm,       a = gamma_D / (2 (1 - gamma_D)).
  Clip coefficient.  q = M / (norm + c), M = the fp32 max_norm, c = the fp32 1e-6f.  The sum norm' + c is rounded (u)
  and norm / (norm + c) <= 1, the quotient is rounded (DIV_REL = u): q' / q <= (1 + u) / ((1 - r_norm)(1 - u)) =
  1 + r_q and q' / q >= 1 - r_q.  min(., 1) is 1-Lipschitz: |coef' - coef| <= r_q q.  Where q (1 - r_q) >= 1 the
  kernel's quotient exceeds 1 as well: the coefficient is EXACTLY 1 (bound 0), as it is for max_norm <= 0.
  Step.  A float that counts: exact below 2^24.
  Bias corrections.  powf(b, t) = b^t (1 + d), |d| <= POW_REL = 2 ulp = 2^-22.  That is a CONDITION on the device's
  powf, not a measurement (the EXP_REL precedent of transformer_pointwise_ref); the GPU test reports what the device
  delivers.  1 - b^t amplifies it by b^t / (1 - b^t) (999 at beta2 = 0.999, t = 1) and rounds once:
      r_1 = (1 + POW_REL b^t / (1 - b^t)) (1 + u) - 1,          |bc1' - bc1| <= r_1 bc1
      |bc2s' - bc2s| <= (a + u + a u) bc2s,  a = r_2 / (2 (1 - r_2))         (the square root halves it, sqrtf adds u)

Elementwise, against fp64 evaluated on the kernel's OWN fp32 p, g, m, v from before the step and the kernel's OWN
coef, bc1, bc2s read back from `state` (`ref_elementwise`): the scalars' error is not inherited, and each step is
compared on its own, so nothing drifts.  With d = gg - m and the fp32 values of 1 - beta (exact for beta >= 1/2, else
their rounding e_b enters):
    g'  = fl(g coef)                          one rounding:       E_g  = u |g_ref|
    gg  = fma(wd, p, g')  (g' if wd = 0)      one more:           E_gg = E_g + u (|gg| + E_g)
    m'  = fma(fl(gg - m), 1 - b1, m)          E_d = E_gg + u (|d| + E_gg);   E_m = X + u (|m_ref| + X),
                                              X = (1 - b1) E_d + e_b1 |d|
    v'  = fma(b2, v, fl(fl((1 - b2) gg) gg))  E_x = (1 - b2) E_gg (2 |gg| + E_gg) + e_b2 gg^2 + 2u (1 - b2)(|gg| + E_gg)^2
                                              E_v = E_x + u (|v_ref| + E_x)
    p'  = p - fl(fl(fl(lr / bc1) m') / fl(fl(sqrtf(v') / bc2s) + eps))
With delta_ref = (lr / bc1) m_ref / (sqrt(v_ref) / bc2s + eps) the fp64 update,
    |p' - p_ref| <= u |p_ref| + K u |delta_ref| + inherited,          K = 7,
K counted from the kernel's operations on delta: the quotient lr / bc1, sqrtf, the divide by bc2s (these two act on
sqrt(v) / bc2s <= the denominator), the add of eps, the multiply by m', the divide, each one correctly rounded (u);
the subtract rounds at |p_ref| + its share of delta, which with all second-order terms is the seventh.  `inherited`
is what m' and v' carry in through delta, to first order (times 1 + 2^-16 for the cross terms):
    (lr / bc1) E_m / den  +  |delta_ref| (E_s / bc2s) / den,   E_s = min(sqrt(E_v), E_v / sqrt(v_ref))
(|sqrt a - sqrt b| <= both).  Where m' and v' are good to a few u of themselves - no cancellation in gg - m - this is
a few u |delta_ref| more; it is never at the parameter's scale.

Planted errors.  `emu_step` is a float32 transcription of the three kernels, operation by operation, sums in the
kernels' order, fma through `_fma32`; its `plant=` makes the deliberately wrong kernel (PLANTS: plant -> the case that
is meant to catch it).  The CPU test proves the bounds accept the emulation on every case and reject every plant.
"""
import collections
import functools
import math

import numpy as np
import torch

from transformer_gemm_ref import NotExercised, TINY, U32, _fma32, check  # noqa: F401

POW_REL = 2.0 ** -22         # condition on powf: 2 ulp
DIV_REL = U32                # IEEE divide
SQRT_REL = U32               # IEEE square root
K_P = 7
CLIP_EPS32 = float(np.float32(1e-6))
OPT_CHUNK, OPT_MAX_T, FIN_THREADS = 4096, 80, 256
ST_STEP, ST_NORM, ST_COEF, ST_BC1, ST_BC2S = 0, 1, 2, 3, 4

Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps wd")


def f32(x):
    return float(np.float32(x))


def hyper32(lr, betas, eps, wd):
    """The values the host passes: every hyper-parameter rounded to fp32."""
    return Hyper(f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(wd))


BENCH = hyper32(1e-4, (0.9, 0.999), 1e-8, 1e-8)      # bench.py
OLD = hyper32(1e-2, (0.9, 0.99), 1e-8, 1e-2)         # tests/test_optim_gpu.py

# plant -> the case that is meant to catch it
PLANTS = collections.OrderedDict((
    ("eps_inside_sqrt", "t80_tiny_norm"),
    ("decay_before_clip", "t80_old_clip_active"),
    ("coef_epsilon_dropped", "t80_tiny_norm"),
    ("bc2_not_rooted", "t1_bench_clip_active"),
    ("bias_correction_previous_step", "t81_loaded1000"),
    ("second_table_partials_overwrite_first", "t81_small_p_clip_inactive"),
    ("finalize_reads_first_256_partials", "t161_big_clip_active"),
    ("tail_element_skipped", "t1_n3_zero_p_clip_off"),
))
BIAS_PLANTS = ("bc2_not_rooted", "bias_correction_previous_step")


def n_partials(sizes):
    return sum(-(-int(n) // OPT_CHUNK) for n in sizes)


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
SIZES8 = (1, 2, 3, 5, 4095, 4096, 4097, 8193)
BIG = 300 * 4096 + 7

# p_scale: |p| around it (0: exactly 0).  g_norm: the total gradient norm is scaled to it (None: randn * g_scale).
# start: completed steps loaded before the first one (0: zero state; else non-zero m, v).
Case = collections.namedtuple("Case", "name sizes p_scale g_scale g_norm max_norm hyper start steps")


def _sizes(count, big_at=None):
    s = [SIZES8[i % 8] for i in range(count)]
    if count > OPT_MAX_T:
        s[-1] = 4097          # the last table's only tensor: two chunks, so that losing its partials shows in the norm
    if big_at is not None:
        s[big_at] = BIG
    return tuple(s)


CASES = [
    Case("t1_bench_clip_active", (4097,), 1.0, 1.0, None, 5.0, BENCH, 0, 3),
    Case("t1_n3_zero_p_clip_off", (3,), 0.0, 1.0, None, 0.0, OLD, 0, 3),
    Case("t80_bench_clip_active", _sizes(80), 1.0, 1.0, None, 5.0, BENCH, 0, 3),
    Case("t80_old_clip_active", _sizes(80), 1.0, 1.0, None, 5.0, OLD, 0, 3),
    Case("t80_tiny_norm", _sizes(80), 1e-3, 1.0, 1e-5, 5e-6, BENCH, 0, 3),
    Case("t81_small_p_clip_inactive", _sizes(81), 1e-3, 1e-3, None, 5.0, BENCH, 0, 3),
    Case("t81_old_zero_p_clip_off", _sizes(81), 0.0, 1.0, None, 0.0, OLD, 0, 3),
    Case("t81_loaded1000", _sizes(81), 1e-3, 1.0, None, 5.0, BENCH, 1000, 1),
    Case("t161_big_clip_active", _sizes(161, big_at=100), 1.0, 1.0, None, 5.0, BENCH, 0, 3),
]
CASE = {c.name: c for c in CASES}
assert [len(c.sizes) for c in CASES] == [1, 1, 80, 80, 80, 81, 81, 81, 161]
assert all(sum(c.sizes) < 300000 for c in CASES[:-1]) and n_partials(CASES[-1].sizes) > 512
assert n_partials(CASES[-1].sizes) % FIN_THREADS != 0

Problem = collections.namedtuple("Problem", "ps ms vs grads")     # grads[step] = the list of that step


@functools.lru_cache(maxsize=None)
def make_problem(name):
    """The case's fp32 parameters, loaded moments and one gradient list per step (numpy, never modified: copy)."""
    c = CASE[name]
    rng = np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))
    r32 = lambda n, s: (rng.standard_normal(n) * s).astype(np.float32)  # noqa: E731
    ps = [r32(n, c.p_scale) for n in c.sizes]
    total = sum(c.sizes)
    grads = []
    for _ in range(c.steps):
        gs = [r32(n, c.g_scale) for n in c.sizes]
        if c.g_norm is not None:
            k = c.g_norm / math.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in gs))
            gs = [(g * k).astype(np.float32) for g in gs]
        grads.append(gs)
    gs_scale = c.g_scale if c.g_norm is None else c.g_norm / math.sqrt(total)
    if c.start:
        ms = [r32(n, 0.1 * gs_scale) for n in c.sizes]
        vs = [((0.5 + rng.random(n)) * gs_scale ** 2 * 1e-4).astype(np.float32) for n in c.sizes]
    else:
        ms = [np.zeros(n, np.float32) for n in c.sizes]
        vs = [np.zeros(n, np.float32) for n in c.sizes]
    for a in ps + ms + vs + [g for gs in grads for g in gs]:
        a.setflags(write=False)
    return Problem(ps, ms, vs, grads)


# ----------------------------------------------------------------------------------------------------------------------
# fp64 reference and bounds
# ----------------------------------------------------------------------------------------------------------------------
Scalars = collections.namedtuple("Scalars", "step norm coef bc1 bc2s bound_norm bound_coef bound_bc1 bound_bc2s")


def sum_depth(nb):
    """Roundings a term of the sum of squares passes through at most (module docstring)."""
    return 16 + 6 + 2 + -(-nb // FIN_THREADS) + 8


def norm_rel(nb):
    D = sum_depth(nb)
    gam = D * U32 / (1.0 - D * U32)
    a = gam / (2.0 * (1.0 - gam))
    return a + SQRT_REL + a * SQRT_REL


def _one_minus_pow(b, t):
    """(b^t, 1 - b^t) in fp64 without the cancellation."""
    if b == 0.0:
        return 0.0, 1.0
    x = t * math.log(b)
    return math.exp(x), -math.expm1(x)


def bias_rel(b, t):
    """Relative bound of the kernel's fp32 1 - powf(b, t)."""
    pw, om = _one_minus_pow(b, t)
    return (1.0 + POW_REL * pw / om) * (1.0 + U32) - 1.0


def ref_scalars(gs, step_before, max_norm, h, clip_eps=CLIP_EPS32):
    """The five state floats of the step after `step_before` completed ones, in fp64 on the fp32 gradients, and their
    bounds."""
    nb = n_partials([g.size for g in gs])
    norm = math.sqrt(math.fsum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in gs))
    rn = norm_rel(nb)
    M = f32(max_norm) if max_norm is not None else 0.0
    if M > 0.0:
        q = M / (norm + clip_eps)
        rq = (1.0 + U32) / ((1.0 - rn) * (1.0 - DIV_REL)) - 1.0
        coef = min(q, 1.0)
        bound_coef = 0.0 if q * (1.0 - rq) >= 1.0 else rq * q
    else:
        coef, bound_coef = 1.0, 0.0
    t = step_before + 1
    bc1 = _one_minus_pow(h.b1, t)[1]
    bc2 = _one_minus_pow(h.b2, t)[1]
    r1, r2 = bias_rel(h.b1, t), bias_rel(h.b2, t)
    a = r2 / (2.0 * (1.0 - r2))
    return Scalars(float(t), norm, coef, bc1, math.sqrt(bc2), rn * norm + TINY, bound_coef, r1 * bc1 + TINY,
                   (a + SQRT_REL + a * SQRT_REL) * math.sqrt(bc2) + TINY)


Elem = collections.namedtuple("Elem", "g m v p delta bound_g bound_m bound_v bound_p")


def _one_minus32(b):
    """(the kernel's fp32 1.f - b, its distance from 1 - b)."""
    om = float(np.float32(1.0) - np.float32(b))
    return om, abs(om - (1.0 - b))


def ref_elementwise(p, g, m, v, coef, bc1, bc2s, h):
    """One tensor (or a concatenation): fp64 g', m', v', p' from the fp32 inputs and the given scalars, and the bounds
    of the module docstring."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    coef, bc1, bc2s = float(coef), float(bc1), float(bc2s)
    om1, e1 = _one_minus32(h.b1)
    om2, e2 = _one_minus32(h.b2)
    g_ref = g * coef
    Eg = U32 * np.abs(g_ref) + TINY
    gg = g_ref + h.wd * p
    Egg = Eg + U32 * (np.abs(gg) + Eg) if h.wd != 0.0 else Eg
    d = gg - m
    Ed = Egg + U32 * (np.abs(d) + Egg)
    m_ref = m + d * (1.0 - h.b1)
    X = om1 * Ed + e1 * np.abs(d)
    Em = X + U32 * (np.abs(m_ref) + X) + TINY
    v_ref = h.b2 * v + (1.0 - h.b2) * gg * gg
    Ex = om2 * Egg * (2.0 * np.abs(gg) + Egg) + e2 * gg * gg + (2.0 * U32 + U32 * U32) * om2 * (np.abs(gg) + Egg) ** 2
    Ev = Ex + U32 * (np.abs(v_ref) + Ex) + TINY
    A = h.lr / bc1
    sv = np.sqrt(v_ref)
    den = sv / bc2s + h.eps
    delta = A * m_ref / den
    p_ref = p - delta
    Es = np.minimum(np.sqrt(Ev), Ev / np.maximum(sv, TINY))
    inherited = (A * Em + np.abs(delta) * Es / bc2s) / den
    Ep = U32 * np.abs(p_ref) + (K_P * U32 * np.abs(delta) + inherited) * (1.0 + 2.0 ** -16) + TINY
    return Elem(g_ref, m_ref, v_ref, p_ref, delta, Eg, Em, Ev, Ep)


def ref_step(ps, gs, ms, vs, step_before, max_norm, h, clip_eps=CLIP_EPS32):
    """One whole step in fp64 (inputs of any float type, taken at their values): -> (ps, gs, ms, vs, Scalars)."""
    sc = ref_scalars(gs, step_before, max_norm, h, clip_eps)
    out = [ref_elementwise(p, g, m, v, sc.coef, sc.bc1, sc.bc2s, h) for p, g, m, v in zip(ps, gs, ms, vs)]
    return [e.p for e in out], [e.g for e in out], [e.m for e in out], [e.v for e in out], sc


# ----------------------------------------------------------------------------------------------------------------------
# the checks of one step (CPU emulation and GPU alike)
# ----------------------------------------------------------------------------------------------------------------------
def _cat(xs):
    return np.concatenate([np.asarray(x).reshape(-1) for x in xs])


def _ratio(got, ref, bound):
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / bound)
    return float(np.max(r)) if r.size else 0.0


def _check(got, ref, bound, what, sizes=None):
    g64 = torch.from_numpy(np.array(got, dtype=np.float64).reshape(-1))
    ref = np.array(ref, dtype=np.float64).reshape(-1)
    bound = np.array(np.broadcast_to(np.asarray(bound, np.float64).reshape(-1), ref.shape))
    try:
        check(g64, torch.from_numpy(ref), torch.from_numpy(bound), what)
    except AssertionError as e:
        if sizes is None:
            raise
        bad = np.flatnonzero(~(np.abs(g64.numpy() - ref) <= bound))
        ends = np.cumsum(sizes)
        i = int(np.searchsorted(ends, bad[0], side="right")) if bad.size else -1
        raise AssertionError("%s [first bad element: tensor %d of %d, n = %d, offset %d]"
                             % (e, i, len(sizes), sizes[i], bad[0] - (ends[i] - sizes[i]))) from None
    return _ratio(got, ref, bound)


def verify_scalars(state, gs, step_before, max_norm, h):
    """`check` of state[0..4] against fp64 on the fp32 gradients; -> {quantity: error / bound}."""
    sc = ref_scalars(gs, step_before, max_norm, h)
    st = np.asarray(state, np.float64)
    assert st[ST_STEP] == sc.step, ("step", st[ST_STEP], sc.step)
    out = {}
    for name, i, ref, bound in (("norm", ST_NORM, sc.norm, sc.bound_norm), ("coef", ST_COEF, sc.coef, sc.bound_coef),
                                ("bc1", ST_BC1, sc.bc1, sc.bound_bc1), ("bc2s", ST_BC2S, sc.bc2s, sc.bound_bc2s)):
        out[name] = _check(st[i:i + 1], np.array([ref]), np.array([bound]), name)
    return out


def verify_elementwise(before, after, state, h):
    """before / after = (ps, gs, ms, vs): lists of fp32 arrays around one step; state: the kernel's own scalars.
    `check` of all four roles of every list member; -> {quantity: worst error / bound}."""
    sizes = [int(np.asarray(p).size) for p in before[0]]
    ref = ref_elementwise(*(_cat(x) for x in before), state[ST_COEF], state[ST_BC1], state[ST_BC2S], h)
    ap, ag, am, av = (_cat(x) for x in after)
    return {"g": _check(ag, ref.g, ref.bound_g, "g", sizes), "m": _check(am, ref.m, ref.bound_m, "m", sizes),
            "v": _check(av, ref.v, ref.bound_v, "v", sizes), "p": _check(ap, ref.p, ref.bound_p, "p", sizes)}


def verify_step(before, after, state, step_before, max_norm, h):
    out = verify_scalars(state, before[1], step_before, max_norm, h)
    out.update(verify_elementwise(before, after, state, h))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# float32 emulation of the three kernels, with planted errors
# ----------------------------------------------------------------------------------------------------------------------
def _t32(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, copy=True).reshape(-1))


_F = lambda s: torch.tensor(s, dtype=torch.float32)  # noqa: E731
_LANE = torch.arange(64)


def pow32_rounded(b, t):
    """powf as a correctly rounded function."""
    return np.float32(float(b) ** float(t))


def emu_partials(gs, plant=None):
    """sqnorm_partials_kernel over the host's tables: the float32 partials buffer (unwritten slots stay 0)."""
    if plant == "second_table_partials_overwrite_first" and len(gs) <= OPT_MAX_T:
        raise NotExercised("one table: block0 is 0 anyway")
    partials = torch.zeros(n_partials([g.size for g in gs]), dtype=torch.float32)
    block0 = 0
    for i0 in range(0, len(gs), OPT_MAX_T):
        b = 0
        for g in gs[i0:i0 + OPT_MAX_T]:
            n = int(g.size)
            nbk = -(-n // OPT_CHUNK)
            pad = torch.zeros(nbk * OPT_CHUNK, dtype=torch.float32)       # fma(0, 0, s) = s: padding changes nothing
            pad[:n] = _t32(g)
            q = pad.view(nbk, 4, 256, 4)                                  # [block, k, thread, j]
            s = torch.zeros(nbk, 256, dtype=torch.float32)
            for k in range(4):
                for j in range(4):
                    s = _fma32(q[:, k, :, j], q[:, k, :, j], s)
            w = s.view(nbk, 4, 64)
            for o in (32, 16, 8, 4, 2, 1):                                # lss_wave_sum
                w = w + w[:, :, _LANE ^ o]
            r = w[:, :, 0]
            partials[block0 + b:block0 + b + nbk] = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
            b += nbk
        if plant != "second_table_partials_overwrite_first":
            block0 += b
    return partials


def emu_finalize(partials, state, max_norm, h, plant=None, pow32=pow32_rounded):
    """clip_finalize_kernel: -> the new float32 state[8]."""
    n = partials.numel()
    if plant == "finalize_reads_first_256_partials":
        if n <= FIN_THREADS:
            raise NotExercised("at most 256 partials: one trip of the strided loop")
        n = FIN_THREADS
    L = -(-n // FIN_THREADS)
    pad = torch.zeros(L * FIN_THREADS, dtype=torch.float32)
    pad[:n] = partials[:n]
    s = torch.zeros(FIN_THREADS, dtype=torch.float32)
    for row in pad.view(L, FIN_THREADS):
        s = s + row
    w = FIN_THREADS // 2
    while w > 0:
        s = s[:w] + s[w:2 * w]
        w //= 2
    norm = torch.sqrt(s[0])
    coef = _F(1.0)
    M = f32(max_norm) if max_norm is not None else 0.0
    if plant == "coef_epsilon_dropped" and not M > 0.0:
        raise NotExercised("no clip")
    if M > 0.0:
        coef = torch.minimum(_F(M) / (norm if plant == "coef_epsilon_dropped" else norm + _F(1e-6)), _F(1.0))
    step = np.float32(state[ST_STEP]) + np.float32(1.0)
    tt = step - np.float32(1.0) if plant == "bias_correction_previous_step" else step
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1 = np.float32(1.0) - np.float32(pow32(np.float32(h.b1), tt))
        bc2 = np.float32(1.0) - np.float32(pow32(np.float32(h.b2), tt))
        bc2s = bc2 if plant == "bc2_not_rooted" else np.sqrt(bc2)
    out = np.array(state, dtype=np.float32, copy=True)
    out[ST_STEP], out[ST_NORM], out[ST_COEF], out[ST_BC1], out[ST_BC2S] = step, float(norm), float(coef), bc1, bc2s
    return out


def emu_update(ps, gs, ms, vs, state, h, plant=None):
    """clip_adam_kernel on every list member: -> (ps, gs, ms, vs) as new float32 numpy arrays."""
    coef, bc1, bc2s = (_F(float(state[i])) for i in (ST_COEF, ST_BC1, ST_BC2S))
    lr, b1, b2, eps, wd = (_F(x) for x in h)
    if plant == "decay_before_clip" and (h.wd == 0.0 or float(coef) == 1.0):
        raise NotExercised("no weight decay or no clip")
    if plant == "eps_inside_sqrt" and h.eps == 0.0:
        raise NotExercised("eps = 0")
    if plant == "tail_element_skipped" and all(p.size % 4 == 0 for p in ps):
        raise NotExercised("every size is a multiple of 4")
    step_size = lr / bc1
    out = [[], [], [], []]
    for p0, g0, m0, v0 in zip(ps, gs, ms, vs):
        p, g, m, v = _t32(p0), _t32(g0), _t32(m0), _t32(v0)
        g2 = g * coef
        if plant == "decay_before_clip":
            gg = _fma32(wd.expand_as(p), p, g) * coef
        else:
            gg = _fma32(wd.expand_as(p), p, g2) if h.wd != 0.0 else g2
        m2 = _fma32(gg - m, (_F(1.0) - b1).expand_as(m), m)
        v2 = _fma32(b2.expand_as(v), v, ((_F(1.0) - b2) * gg) * gg)
        if plant == "eps_inside_sqrt":
            den = torch.sqrt(v2 / (bc2s * bc2s) + eps)
        else:
            den = torch.sqrt(v2) / bc2s + eps
        p2 = p - step_size * m2 / den
        new = [p2, g2, m2, v2]
        if plant == "tail_element_skipped" and p.numel() % 4:
            k = p.numel() - p.numel() % 4
            for a, old in zip(new, (p, g, m, v)):
                a[k:] = old[k:]
        for lst, a, src in zip(out, new, (p0, g0, m0, v0)):
            lst.append(a.numpy().reshape(np.asarray(src).shape))
    return tuple(out)


def emu_step(ps, gs, ms, vs, state, max_norm, h, plant=None, pow32=pow32_rounded):
    """The three kernels in float32: -> (ps, gs, ms, vs, state), all new.  `plant`: one of PLANTS."""
    assert plant is None or plant in PLANTS, plant
    partials = emu_partials(gs, plant)
    state = emu_finalize(partials, state, max_norm, h, plant, pow32)
    return emu_update(ps, gs, ms, vs, state, h, plant) + (state,)


def run_case(name, stepper, upto=None):
    """Drives `stepper(ps, gs, ms, vs, state, max_norm, hyper) -> (ps, gs, ms, vs, state)` through the case's steps and
    yields (step index, before, after, state, step_before) of each for `verify_step`."""
    c, pr = CASE[name], make_problem(name)
    ps, ms, vs = pr.ps, pr.ms, pr.vs
    state = np.zeros(8, np.float32)
    state[ST_STEP] = c.start
    for k, gs in enumerate(pr.grads[:upto]):
        before = (ps, gs, ms, vs)
        step_before = int(state[ST_STEP])
        ps, g2, ms, vs, state = stepper(ps, gs, ms, vs, state, c.max_norm, c.hyper)
        yield k, before, (ps, g2, ms, vs), state, step_before
