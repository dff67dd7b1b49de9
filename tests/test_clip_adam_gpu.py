"""K10 on the GPU (csrc/optim.hip, optim.ClipAdam) against fp64 with the derived bounds of tests/clip_adam_ref.py, one
step at a time: every case of the helper through `lss_clip_adam_step` and through `ClipAdam`, the same lists as
unaligned views of flat buffers (the scalar paths), a real `dp.GradBucket` driven through `dp._clip_and_step`, the
Python logic of `ClipAdam.step`, and a graph replay that holds three tables."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_adam_ref as R  # noqa: E402
from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import dp  # noqa: E402
from lss2_multimodal_nu_amd.optim import ClipAdam, _OptTensor  # noqa: E402

PAD = -7.5e33                    # guard value: nothing the step computes
NAMES = [c.name for c in R.CASES]
QUANTITIES = ("norm", "coef", "bc1", "bc2s", "g", "m", "v", "p")


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def _guards_intact(buf, spans):
    """Every element of `buf` outside the [lo, hi) spans still holds PAD, bit for bit."""
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for lo, hi in spans:
        keep[lo:hi] = False
    return bool((buf[keep] == torch.full((), PAD, device=buf.device)).all()) and int(keep.sum()) > 0


def raw_step(entries, state, max_norm, h):
    """`lss_clip_adam_step` on [(p, g, m, v)] device tensors; the partials buffer sits between guard words."""
    sizes = [p.numel() for p, _, _, _ in entries]
    nb = int(N.lib().lss_clip_adam_partials((ctypes.c_longlong * len(sizes))(*sizes), len(sizes)))
    assert nb == R.n_partials(sizes)
    G = 64
    pbuf = torch.full((G + nb + G,), PAD, dtype=torch.float32, device="cuda")
    tab = (_OptTensor * len(entries))()
    for i, (p, g, m, v) in enumerate(entries):
        assert all(t.is_contiguous() and t.dtype == torch.float32 and t.numel() == p.numel() for t in (p, g, m, v))
        tab[i].p, tab[i].g, tab[i].m, tab[i].v, tab[i].n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    N.check(N.lib().lss_clip_adam_step(ctypes.cast(tab, ctypes.c_void_p), len(entries), state.data_ptr(),
                                       pbuf.data_ptr() + 4 * G, nb, h.lr, h.b1, h.b2, h.eps, h.wd,
                                       float(max_norm or 0.0), N.stream()), "lss_clip_adam_step")
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, [(G, G + nb)]), "the partials' guard words were written"


class Flat:
    """One role's list members back to back in one flat buffer, no padding: 3 guard elements in front, 5 between
    members `gap` and `gap + 1`, 7 behind.  Allocations are 512-byte aligned, so a member is 16-byte aligned exactly
    where its element offset is a multiple of 4."""
    FRONT, GAP, TAIL = 3, 5, 7

    def __init__(self, arrays):
        gap = len(arrays) // 2
        self.spans, o = [], self.FRONT
        for i, a in enumerate(arrays):
            self.spans.append((o, o + a.size))
            o += a.size + (self.GAP if i == gap and i + 1 < len(arrays) else 0)
        host = np.full(o + self.TAIL, PAD, np.float32)
        for (lo, hi), a in zip(self.spans, arrays):
            host[lo:hi] = a.reshape(-1)
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[lo:hi] for lo, hi in self.spans]

    def unaligned(self):
        return sum(v.data_ptr() % 16 != 0 for v in self.views)


def make_stepper(unaligned=()):
    """A `run_case` stepper on the raw entry; roles named in `unaligned` ('p', 'g', 'm', 'v') live in a `Flat`."""
    def step(ps, gs, ms, vs, state, max_norm, h):
        roles, flats = {}, []
        for key, arrays in zip("pgmv", (ps, gs, ms, vs)):
            if key in unaligned:
                f = Flat(arrays)
                assert len(arrays) < 3 or f.unaligned() * 2 > len(arrays)      # most members are unaligned
                flats.append(f)
                roles[key] = f.views
            else:
                roles[key] = [_dev(a) for a in arrays]
                assert all(t.data_ptr() % 16 == 0 for t in roles[key])
        st = _dev(state)
        raw_step(list(zip(roles["p"], roles["g"], roles["m"], roles["v"])), st, max_norm, h)
        for f in flats:
            assert _guards_intact(f.buf, f.spans), "bytes between or around the members were written"
        back = lambda ts, like: [t.cpu().numpy().reshape(np.asarray(a).shape) for t, a in zip(ts, like)]  # noqa: E731
        return back(roles["p"], ps), back(roles["g"], gs), back(roles["m"], ms), back(roles["v"], vs), st.cpu().numpy()
    return step


def _verify_case(name, stepper, report, tag, upto=None):
    """Every step of the case: snapshot, one step, read back, `check` scalars and all four roles of every member."""
    c = R.CASE[name]
    worst, trail = dict.fromkeys(QUANTITIES, 0.0), []
    for k, before, after, state, step_before in R.run_case(name, stepper, upto):
        ratios = R.verify_step(before, after, state, step_before, c.max_norm, c.hyper)
        for q, r in ratios.items():
            worst[q] = max(worst[q], r)
        if not c.max_norm > 0:
            assert state[R.ST_COEF] == 1.0
        trail.append((before, after, state, step_before))
    for q in QUANTITIES:
        assert report("clip_adam/%s/%s/%s_err_over_bound" % (tag, name, q), worst[q]) <= 1.0
    return trail


def _clip_adam_on(before, c, step_before):
    """The same step through optim.ClipAdam: -> (after, state)."""
    ps, gs, ms, vs = before
    params = [torch.nn.Parameter(_dev(p)) for p in ps]
    h = c.hyper
    opt = ClipAdam(params, lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd,
                   max_grad_norm=c.max_norm if c.max_norm > 0 else None)
    for p, g, m, v in zip(params, gs, ms, vs):
        p.grad = _dev(g)
        if step_before:       # a loaded checkpoint: torch.optim.Adam's per-parameter layout
            opt.state[p] = {"step": torch.tensor(float(step_before)), "exp_avg": _dev(m), "exp_avg_sq": _dev(v)}
    opt.step()
    torch.cuda.synchronize()
    host = lambda ts: [t.detach().cpu().numpy() for t in ts]  # noqa: E731
    return (host(params), host([p.grad for p in params]), host([opt.state[p]["exp_avg"] for p in params]),
            host([opt.state[p]["exp_avg_sq"] for p in params])), opt._dev[params[0].device][0].cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_every_case_against_fp64(name, report):
    """The raw entry on aligned tensors, every step; `ClipAdam` on each step's own inputs gives the same bits (same
    kernels, same alignment) - from zero state for the first step and from loaded moments and step count after it."""
    c = R.CASE[name]
    trail = _verify_case(name, make_stepper(), report, "raw")
    for before, after, state, step_before in trail:
        got, st = _clip_adam_on(before, c, step_before)
        assert np.array_equal(st[:5], state[:5])
        assert all(np.array_equal(a, b) for x, y in zip(got, after) for a, b in zip(x, y))
        if name in ("t1_bench_clip_active", "t81_loaded1000"):
            # beta2 = 0.999: what powf and the cancellation deliver on this device, raw (the bound's condition is POW_REL)
            sc = R.ref_scalars(before[1], step_before, c.max_norm, c.hyper)
            report("clip_adam/bias/bc1_rel_err_step%d" % sc.step, abs(float(state[R.ST_BC1]) - sc.bc1) / sc.bc1)
            report("clip_adam/bias/bc2s_rel_err_step%d" % sc.step, abs(float(state[R.ST_BC2S]) - sc.bc2s) / sc.bc2s)
            report("clip_adam/bias/bc2s_bound_rel_step%d" % sc.step, sc.bound_bc2s / sc.bc2s)


@pytest.mark.parametrize("roles", ["g", "pgmv"])
@pytest.mark.parametrize("name", NAMES)
def test_unaligned_views_take_the_scalar_paths(name, roles, report):
    """'g': only the gradients are views of a flat buffer (dp.GradBucket's situation: the sum of squares and the update
    both leave their float4 path); 'pgmv': all four.  Same bounds; the guard elements keep their bits."""
    c = R.CASE[name]
    _verify_case(name, make_stepper(unaligned=roles), report, "unaligned_" + roles, upto=None if c.steps == 1 else 2)


# ----------------------------------------------------------------------------------------------------------------------
# a real GradBucket through dp._clip_and_step
# ----------------------------------------------------------------------------------------------------------------------
BUCKET_SIZES = (1, 3, 5, 17, 64, 130, 257, 1000, 4097)


def test_grad_bucket_through_clip_and_step(report):
    """90 parameters whose `.grad` are views of one flat buffer (n_buckets = 3, one process, no collective).  Step 1
    uses every parameter, step 2 leaves two out: `hide_unused()` drops them from the optimizer's list."""
    gen = torch.Generator().manual_seed(90)
    sizes = [BUCKET_SIZES[i % len(BUCKET_SIZES)] for i in range(90)]
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 1e-3).cuda()) for n in sizes]
    weights = [[torch.randn(n, generator=gen).cuda() for n in sizes] for _ in range(2)]
    bucket = dp.GradBucket(params, n_buckets=3)
    assert len(bucket.buckets) == 3 and sum(bucket.views[p].data_ptr() % 16 != 0 for p in params) > 45
    h = R.BENCH
    opt = ClipAdam(params, lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd)
    offset, o = {}, 0
    for p in reversed(params):            # the bucket's layout: reverse registration order, no padding
        offset[p] = o
        o += p.numel()
    host = lambda ts: [t.detach().cpu().numpy().copy() for t in ts]  # noqa: E731
    moments = lambda key, ps: [opt.state[p][key] if opt.state[p] else torch.zeros_like(p) for p in ps]  # noqa: E731
    hidden = [params[7], params[40]]
    for step, idx in enumerate([list(range(90)), [i for i in range(90) if i not in (7, 40)]]):
        active = [params[i] for i in idx]
        bucket.zero()
        sum((params[i] * weights[step][i]).sum() for i in idx).backward()
        assert all(p.grad is bucket.views[p] for p in params)
        before = (host(active), host([p.grad for p in active]), host(moments("exp_avg", active)),
                  host(moments("exp_avg_sq", active)))
        assert all(np.array_equal(g, weights[step][i].cpu().numpy()) for g, i in zip(before[1], idx))
        frozen = [host([p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]) for p in hidden] if step else None
        dp._clip_and_step(opt, bucket, None, 5.0)
        torch.cuda.synchronize()
        assert all(p.grad is bucket.views[p] for p in params)
        flat = bucket.flat.cpu().numpy()
        after = (host(active), [flat[offset[p]:offset[p] + p.numel()] for p in active],    # the clipped g is IN the buffer
                 host(moments("exp_avg", active)), host(moments("exp_avg_sq", active)))
        state = opt._dev[params[0].device][0].cpu().numpy()
        assert float(opt.grad_norm) == float(state[R.ST_NORM]) == float(dp._last_norm[0])
        ratios = R.verify_step(before, after, state, step, 5.0, h)
        assert state[R.ST_COEF] < 0.1                                                       # the clip is active
        for q, r in ratios.items():
            assert report("clip_adam/grad_bucket/step%d/%s_err_over_bound" % (step + 1, q), r) <= 1.0
        if step:
            for p, was in zip(hidden, frozen):
                now = host([p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]])
                assert all(np.array_equal(a, b) for a, b in zip(now, was)), "a hidden parameter was touched"
                assert not flat[offset[p]:offset[p] + p.numel()].any()


# ----------------------------------------------------------------------------------------------------------------------
# the Python logic of ClipAdam.step
# ----------------------------------------------------------------------------------------------------------------------
def _small(k=0):
    """The first eight tensors of a case (sizes 1 .. 8193): parameters and the gradients of step k."""
    pr = R.make_problem("t80_old_clip_active")
    return pr.ps[:8], pr.grads[k][:8]


def _params(ps, gs):
    out = [torch.nn.Parameter(_dev(p)) for p in ps]
    for p, g in zip(out, gs):
        if g is not None:
            p.grad = _dev(g)
    return out


def _kw(h):
    return dict(lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd)


def _state(opt, params):
    return opt._dev[params[0].device][0].cpu().numpy()


@pytest.mark.parametrize("ctor,call,effective", [(None, 0.5, 0.5), (5.0, 0.5, 0.5), (0.5, None, 0.5), (5.0, 0.0, 0.0),
                                                 (None, None, 0.0)])
def test_max_grad_norm_of_the_call_overrides_the_constructors(ctor, call, effective):
    ps, gs = _small()
    params = _params(ps, gs)
    opt = ClipAdam(params, max_grad_norm=ctor, **_kw(R.OLD))
    opt.step(max_grad_norm=call)
    torch.cuda.synchronize()
    st = _state(opt, params)
    R.verify_scalars(st, gs, 0, effective, R.OLD)
    assert (st[R.ST_COEF] == 1.0) == (effective == 0.0)
    z = [np.zeros_like(p) for p in ps]
    after = tuple([t.detach().cpu().numpy() for t in ts] for ts in
                  (params, [p.grad for p in params], [opt.state[p]["exp_avg"] for p in params],
                   [opt.state[p]["exp_avg_sq"] for p in params]))
    R.verify_elementwise((ps, gs, z, z), after, st, R.OLD)


def test_groups_with_equal_hyper_parameters_equal_one_group_and_differing_ones_are_refused():
    ps, gs = _small()
    one = _params(ps, gs)
    two = _params(ps, gs)
    a = ClipAdam(one, max_grad_norm=5.0, **_kw(R.OLD))
    b = ClipAdam([dict(params=two[:3]), dict(params=two[3:])], max_grad_norm=5.0, **_kw(R.OLD))
    for k in range(2):
        for p, q, g in zip(one, two, R.make_problem("t80_old_clip_active").grads[k][:8]):
            p.grad, q.grad = _dev(g), _dev(g)
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) and torch.equal(p.grad, q.grad) for p, q in zip(one, two))
    assert np.array_equal(_state(a, one)[:5], _state(b, two)[:5]) and _state(b, two)[0] == 2.0
    # differing groups: refused before anything is written - parameters, gradients, moments and the step count
    for key, val in (("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-6), ("weight_decay", 0.0)):
        bad = _params(ps, gs)
        opt = ClipAdam([dict(params=bad[:3]), dict(params=bad[3:], **{key: val})], max_grad_norm=5.0, **_kw(R.OLD))
        with pytest.raises(ValueError):
            opt.step()
        torch.cuda.synchronize()
        assert all(np.array_equal(p.detach().cpu().numpy(), p0) and np.array_equal(p.grad.cpu().numpy(), g0)
                   for p, p0, g0 in zip(bad, ps, gs)), key
        assert all(not bool(t.any()) for p in bad for k, t in opt.state[p].items() if k != "step"), key
        assert all(float(st[0][0]) == 0.0 for st in opt._dev.values()), key


def test_partials_buffer_grows_and_the_step_count_continues():
    """Step 1 sees two small tensors (2 partials), step 2 all eight (11): the partials buffer is replaced, the state
    floats are not, and step 2 is the second step - bias corrections and all - within the bounds."""
    ps, g0 = _small(0)
    _, g1 = _small(1)
    params = _params(ps, [g0[0], g0[1]] + [None] * 6)
    opt = ClipAdam(params, max_grad_norm=5.0, **_kw(R.OLD))
    opt.step()
    torch.cuda.synchronize()
    dev = params[0].device
    state_t, part_t = opt._dev[dev]
    assert part_t.numel() == 2 and float(state_t[0]) == 1.0
    assert all(torch.equal(p.detach(), _dev(p0)) and not opt.state[p] for p, p0 in zip(params[2:], ps[2:]))
    host = lambda ts: [t.detach().cpu().numpy().copy() for t in ts]  # noqa: E731
    for p, g in zip(params, g1):
        p.grad = _dev(g)
    m0 = host([opt.state[p]["exp_avg"] if opt.state[p] else torch.zeros_like(p) for p in params])
    v0 = host([opt.state[p]["exp_avg_sq"] if opt.state[p] else torch.zeros_like(p) for p in params])
    before = (host(params), g1, m0, v0)
    assert m0[0].any() and not m0[2].any()
    opt.step()
    torch.cuda.synchronize()
    assert opt._dev[dev][0] is state_t and opt._dev[dev][1] is not part_t and opt._dev[dev][1].numel() >= R.n_partials([p.size for p in ps])
    after = (host(params), host([p.grad for p in params]), host([opt.state[p]["exp_avg"] for p in params]),
             host([opt.state[p]["exp_avg_sq"] for p in params]))
    st = state_t.cpu().numpy()
    assert st[0] == 2.0 and all(float(opt.state[p]["step"]) == 2.0 for p in params)
    R.verify_step(before, after, st, 1, 5.0, R.OLD)


def test_graph_replay_with_three_tables_equals_eager():
    """161 tensors, 522 partials: the capture holds three launches of each list kernel, with their `block0` offsets
    and by-value tables, and the finalize's third trip; two replays == two eager steps, bit for bit."""
    pr = R.make_problem("t161_big_clip_active")
    h = R.BENCH

    def run(graphed):
        ps = [torch.nn.Parameter(_dev(p)) for p in pr.ps]
        static_g = [torch.zeros_like(p) for p in ps]
        for p, g in zip(ps, static_g):
            p.grad = g
        opt = ClipAdam(ps, max_grad_norm=5.0, **_kw(h))
        load = lambda gs: [g.copy_(_dev(src)) for g, src in zip(static_g, gs)]  # noqa: E731
        load(pr.grads[0])
        opt.step()            # warm-up step (state allocation) outside the capture
        graph = None
        if graphed:
            load(pr.grads[1])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
        for gs in pr.grads[1:]:
            load(gs)
            graph.replay() if graphed else opt.step()
        torch.cuda.synchronize()
        return [p.detach().clone() for p in ps] + [opt._dev[ps[0].device][0].clone()]

    a, b = run(False), run(True)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and float(a[-1][0]) == 3.0
