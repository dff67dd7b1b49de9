"""CPU checks of tests/clip_adam_ref.py itself and of K10's C ABI without a launch: the fp64 reference against torch's
own float64 clip + Adam, the float32 emulation of the three kernels inside the derived bounds on every case, every
planted error outside them (by name, on the case that is meant to catch it), the conditions the bounds rest on, and the
argument checks of `lss_clip_adam_partials` / `lss_clip_adam_step` (only refused calls are made: nothing is launched)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import clip_adam_ref as R

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
NAMES = [c.name for c in R.CASES]


# ----------------------------------------------------------------------------------------------------------------------
# the reference is torch's clip_grad_norm_ + Adam
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.start == 0])
def test_reference_equals_torch_in_float64(name):
    """Same fp32-rounded hyper-parameters on both sides; 1e-12 relative on every tensor after each of 3 steps.  torch's
    clip adds the double 1e-6, the kernel the float 1e-6f (2.5e-15 apart: 2e-10 of the tiny-norm case's norm), so this
    comparison alone hands the reference torch's constant."""
    c, pr = R.CASE[name], R.make_problem(name)
    h = c.hyper
    tp = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in pr.ps]
    opt = torch.optim.Adam(tp, lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd)
    ps, ms, vs = pr.ps, pr.ms, pr.vs
    close = lambda a, b: float(np.abs(a - b).max()) <= 1e-12 * float(np.abs(b).max())  # noqa: E731
    for k, gs in enumerate(pr.grads):
        for q, g in zip(tp, gs):
            q.grad = torch.from_numpy(g.astype(np.float64))
        if c.max_norm > 0:
            norm_t = float(torch.nn.utils.clip_grad_norm_(tp, R.f32(c.max_norm)))
        opt.step()
        ps, g2, ms, vs, sc = R.ref_step(ps, gs, ms, vs, k, c.max_norm, h, clip_eps=1e-6)
        if c.max_norm > 0:
            assert abs(sc.norm - norm_t) <= 1e-12 * norm_t
        for i, q in enumerate(tp):
            st = opt.state[q]
            assert close(ps[i], q.detach().numpy()), (k, i, "p")
            assert close(g2[i], q.grad.numpy()), (k, i, "g")
            assert close(ms[i], st["exp_avg"].numpy()) and close(vs[i], st["exp_avg_sq"].numpy()), (k, i, "m, v")
    assert float(opt.state[tp[0]]["step"]) == sc.step == len(pr.grads)


# ----------------------------------------------------------------------------------------------------------------------
# the emulation passes, the plants do not
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clean(name):
    """The emulation's own trajectory: [(before, after, state_before, state_after, step_before)] per step."""
    out, state0 = [], np.zeros(8, np.float32)
    state0[R.ST_STEP] = R.CASE[name].start
    for k, before, after, state, step_before in R.run_case(name, R.emu_step):
        out.append((before, after, state0, state, step_before))
        state0 = state
    return out


@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_inside_every_bound(name):
    c = R.CASE[name]
    for before, after, _, state, step_before in _clean(name):
        ratios = R.verify_step(before, after, state, step_before, c.max_norm, c.hyper)
        print(name, "step", step_before + 1, " ".join("%s %.3f" % kv for kv in sorted(ratios.items())))
        assert all(r <= 1.0 for r in ratios.values())
        if not c.max_norm > 0:
            assert state[R.ST_COEF] == 1.0
            assert all(np.array_equal(a, b) for a, b in zip(after[1], before[1]))    # clip off: g is not changed


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _plant_step(name, k, plant, pow32=R.pow32_rounded):
    """Step k of the case from the clean state with the plant: was it rejected?  (NotExercised passes through.)"""
    c = R.CASE[name]
    before, _, state0, _, step_before = _clean(name)[k]
    *after, state = R.emu_step(*before, state0, c.max_norm, c.hyper, plant=plant, pow32=pow32)
    return _rejected(lambda: R.verify_step(before, tuple(after), state, step_before, c.max_norm, c.hyper))


def plant_verdicts(plant):
    """{(case, step): rejected?} over every case that exercises the plant; none at all: NotExercised."""
    out = {}
    for c in R.CASES:
        steps = range(c.steps) if len(c.sizes) <= 81 else (0,)      # the long list: its first step is enough
        for k in steps:
            try:
                out[(c.name, c.start + k + 1)] = _plant_step(c.name, k, plant)
            except R.NotExercised:
                pass
    if not out:
        raise R.NotExercised("no case exercises %s" % plant)
    return out


@pytest.mark.parametrize("plant", list(R.PLANTS))
def test_plant_is_rejected(plant):
    v = plant_verdicts(plant)
    print(plant, "rejected on", sorted(k for k, r in v.items() if r), "accepted on", sorted(k for k, r in v.items() if not r))
    meant = [r for (name, _), r in v.items() if name == R.PLANTS[plant]]
    assert meant and all(meant), "%s is not rejected on every step of %s" % (plant, R.PLANTS[plant])


def test_a_plant_no_case_exercises_is_not_passed_silently(monkeypatch):
    monkeypatch.setattr(R, "CASES", [c for c in R.CASES if len(c.sizes) <= R.OPT_MAX_T])
    with pytest.raises(R.NotExercised):
        plant_verdicts("second_table_partials_overwrite_first")
    monkeypatch.setattr(R, "CASES", [R.CASE["t1_n3_zero_p_clip_off"]])
    for plant in ("coef_epsilon_dropped", "decay_before_clip", "finalize_reads_first_256_partials"):
        with pytest.raises(R.NotExercised):
            plant_verdicts(plant)


def test_the_planted_quantities_are_the_ones_that_fail():
    """Each plant moves what it is meant to move on its case, not something else."""
    def failing(plant, k=0):
        name = R.PLANTS[plant]
        c = R.CASE[name]
        before, _, state0, _, step_before = _clean(name)[k]
        *after, state = R.emu_step(*before, state0, c.max_norm, c.hyper, plant=plant)
        bad = set()
        sc = R.ref_scalars(before[1], step_before, c.max_norm, c.hyper)
        for q, i, ref, bound in (("norm", 1, sc.norm, sc.bound_norm), ("coef", 2, sc.coef, sc.bound_coef),
                                 ("bc1", 3, sc.bc1, sc.bound_bc1), ("bc2s", 4, sc.bc2s, sc.bound_bc2s)):
            if not abs(float(state[i]) - ref) <= bound:
                bad.add(q)
        if np.isfinite(state[:5]).all() and state[R.ST_BC1] > 0 and state[R.ST_BC2S] > 0:
            ref = R.ref_elementwise(*(R._cat(x) for x in before), state[2], state[3], state[4], c.hyper)
            for q, got, r, b in (("g", after[1], ref.g, ref.bound_g), ("m", after[2], ref.m, ref.bound_m),
                                 ("v", after[3], ref.v, ref.bound_v), ("p", after[0], ref.p, ref.bound_p)):
                if not bool((np.abs(R._cat(got).astype(np.float64) - r) <= b).all()):
                    bad.add(q)
        return bad

    assert failing("eps_inside_sqrt") == {"p"}
    assert failing("decay_before_clip") == {"m", "v", "p"}
    assert failing("coef_epsilon_dropped") == {"coef"}
    assert failing("bc2_not_rooted") == {"bc2s"}
    assert failing("bias_correction_previous_step") == {"bc2s"}       # 0.9^1000 = 0: bc1 is 1 either way
    assert failing("second_table_partials_overwrite_first") >= {"norm"}
    assert failing("finalize_reads_first_256_partials") >= {"norm"}
    assert failing("tail_element_skipped") == {"m", "v", "p"}         # clip off: g stays as it is anyway


# ----------------------------------------------------------------------------------------------------------------------
# the conditions the bias-correction bound rests on
# ----------------------------------------------------------------------------------------------------------------------
def _shifted(ulps):
    """A powf that is off by `ulps` units in the last place on top of its rounding: within POW_REL for |ulps| <= 1."""
    def pw(b, t):
        r = R.pow32_rounded(b, t)
        for _ in range(abs(ulps)):
            r = np.nextafter(r, np.float32(2.0 if ulps > 0 else 0.0))
        return r
    return pw


def _bias_state(h, t, pow32):
    st = np.zeros(8, np.float32)
    st[R.ST_STEP] = t - 1
    return R.emu_finalize(torch.ones(1), st, 0.0, h, None, pow32)


@pytest.mark.parametrize("h", [R.BENCH, R.OLD], ids=["bench", "old"])
@pytest.mark.parametrize("t", [1, 2, 3, 10, 100, 1001, 20000])
def test_pow_condition(h, t):
    """A powf within POW_REL = 2 ulp stays inside the bias-correction bounds (1 ulp off plus its own rounding is 1.5);
    one that is 4 ulp off does not at beta2 = 0.999, t = 1, where the bound is tightest in ulps of 1 - b^t.  numpy's own
    float32 power stays inside: a sanity check of the bound, not a statement about the device."""
    sc = R.ref_scalars([np.ones(1, np.float32)], t - 1, 0.0, h)
    inside = lambda st: (abs(float(st[3]) - sc.bc1) <= sc.bound_bc1 and  # noqa: E731
                         abs(float(st[4]) - sc.bc2s) <= sc.bound_bc2s)
    for pw in (R.pow32_rounded, _shifted(1), _shifted(-1), lambda b, t: np.power(np.float32(b), np.float32(t))):
        assert inside(_bias_state(h, t, pw)), (h, t)
    if t == 1:
        assert not inside(_bias_state(h, t, _shifted(4))) and not inside(_bias_state(h, t, _shifted(-4)))


@pytest.mark.parametrize("plant", R.BIAS_PLANTS)
@pytest.mark.parametrize("ulps", [1, -1])
def test_bias_plants_are_rejected_under_the_pow_condition(plant, ulps):
    """POW_REL leaves no room for a wrong bias correction: with a powf at the edge of the condition, in the direction
    that helps or hurts, both plants are still rejected on their cases - at steps 1, 2, 3 and 1001."""
    for name in sorted(set(R.PLANTS[p] for p in R.BIAS_PLANTS)):
        for k in range(R.CASE[name].steps):
            assert _plant_step(name, k, plant, _shifted(ulps)), (plant, name, k)


def test_bounds_are_at_the_updates_scale():
    """What the earlier test could not see: at lr = 1e-4 and |p| around 1 the bound of p' allows an error of the UPDATE
    of a few parts in 10^5 at most, where 5e-6 max|q| allowed 20 %; with |p| <= 1e-3 or p = 0 it is parts in 10^6."""
    for name, cap in (("t80_bench_clip_active", 1e-3), ("t81_small_p_clip_inactive", 3e-6), ("t81_old_zero_p_clip_off", 3e-6)):
        c = R.CASE[name]
        before, _, _, state, _ = _clean(name)[0]
        ref = R.ref_elementwise(*(R._cat(x) for x in before), state[2], state[3], state[4], c.hyper)
        rel = ref.bound_p / np.abs(ref.delta)
        print(name, "median bound / |delta| %.2e" % float(np.median(rel)))
        assert float(np.median(rel)) <= cap
    assert R.sum_depth(522) == 35 and R.sum_depth(256) == 33 and R.norm_rel(522) < 19 * R.U32


# ----------------------------------------------------------------------------------------------------------------------
# C ABI without a launch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from lss2_multimodal_nu_amd import _native, build_native
    build_native.build(verbose=False)
    return _native.lib()


def _sizes_arr(sizes):
    return (ctypes.c_longlong * len(sizes))(*sizes)


def test_partials_count(L):
    for c in R.CASES:
        assert L.lss_clip_adam_partials(_sizes_arr(c.sizes), len(c.sizes)) == R.n_partials(c.sizes)
    assert R.n_partials(R.CASE["t161_big_clip_active"].sizes) == 522
    assert L.lss_clip_adam_partials(_sizes_arr((4096, 4097, 1)), 3) == 4
    assert L.lss_clip_adam_partials(_sizes_arr((1 << 40,)), 1) == 1 << 28
    assert L.lss_clip_adam_partials(_sizes_arr((5,)), 0) == 0 and L.lss_clip_adam_partials(None, 3) == 0
    assert L.lss_clip_adam_partials(_sizes_arr((5, 0, 7)), 3) == 0 and L.lss_clip_adam_partials(_sizes_arr((5, -4096)), 2) == 0


A = 1 << 20   # an aligned address that is never dereferenced: every call below is refused before any launch


def _step(L, ptrs=((A, A, A, A, 5000),), table=True, count=None, state=A, partials=A, n_partials=None,
          lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, max_norm=5.0):
    from lss2_multimodal_nu_amd.optim import _OptTensor
    tab = (_OptTensor * max(len(ptrs), 1))()
    for i, (p, g, m, v, n) in enumerate(ptrs):
        tab[i].p, tab[i].g, tab[i].m, tab[i].v, tab[i].n = p, g, m, v, n
    if n_partials is None:
        n_partials = R.n_partials([t[4] for t in ptrs if t[4] > 0])
    return L.lss_clip_adam_step(ctypes.cast(tab, ctypes.c_void_p) if table else None, len(ptrs) if count is None else count,
                                ctypes.c_void_p(state), ctypes.c_void_p(partials), n_partials, lr, b1, b2, eps, wd,
                                max_norm, None)


def test_step_argument_checks(L):
    assert _step(L, table=False) == E_NULL
    assert _step(L, state=None) == E_NULL
    assert _step(L, partials=None) == E_NULL
    assert _step(L, count=0) == E_SHAPE and _step(L, count=-1) == E_SHAPE
    for k in range(4):                                 # a null member pointer, in the first and in a later entry
        t = [A, A, A, A, 5000]
        t[k] = None
        assert _step(L, ptrs=(tuple(t),)) == E_NULL, k
        assert _step(L, ptrs=((A, A, A, A, 8), tuple(t))) == E_NULL, k
    assert _step(L, ptrs=((A, A, A, A, 0),), n_partials=0) == E_SHAPE
    assert _step(L, ptrs=((A, A, A, A, -1),), n_partials=0) == E_SHAPE
    assert _step(L, ptrs=((A, A, A, A, 1 << 40),), n_partials=1 << 28) == E_SHAPE
    for k in range(4):                                 # fp32 tensors: 4-byte alignment is all that is asked
        for off in (1, 2, 3):
            t = [A, A, A, A, 5000]
            t[k] = A + off
            assert _step(L, ptrs=(tuple(t),)) == E_ALIGN, (k, off)
    assert _step(L, n_partials=1) == E_SHAPE and _step(L, n_partials=3) == E_SHAPE and _step(L, n_partials=0) == E_SHAPE
    assert _step(L, b1=1.0) == E_SHAPE and _step(L, b2=1.0) == E_SHAPE
    assert _step(L, b1=-0.1) == E_SHAPE and _step(L, b2=float("nan")) == E_SHAPE
    assert _step(L, lr=-1e-4) == E_SHAPE and _step(L, lr=float("nan")) == E_SHAPE
    assert _step(L, eps=-1e-8) == E_SHAPE and _step(L, eps=float("nan")) == E_SHAPE
