"""The forward convs of the tile kernel (csrc/conv_mfma.hip: every reachable conv_lds_kernel instantiation and
conv_direct_kernel) and of the ring kernel (csrc/conv_ring.hip: all six instantiations) alone, per element, against fp64.

References, cases, bounds and the dispatch each case must reach: tests/conv_fwd_ref.py.  The exact cases (integer and
dyadic operands) must equal the fp64 reference rounded once to the output type bit for bit; the bound cases must lie
inside an elementwise bound DERIVED there (u, a count of operations, a magnitude sum, the pinned blended operands);
nothing is taken from a kernel.  Every measured error of a bound case is `report`ed under conv_fwd.*."""
import functools

import pytest
import torch

import conv_fwd_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import ops  # noqa: E402

SWITCHES = ("LSS_CONV_RT", "LSS_CONV_KC", "LSS_CONV_KSPLIT", "LSS_CONV_SRC", "LSS_CONV_WT", "LSS_CONV_DIRECT",
            "LSS_CONV_RING")
_id = lambda c: c.name  # noqa: E731


@functools.lru_cache(maxsize=None)
def _device(name):
    """Device copies of a case's operands and its packed weight: made once, shared, never written to."""
    c = R.BY_NAME[name]
    dev = {k: (None if v is None else v.cuda()) for k, v in R.make_inputs(name).items()}
    w = dev["w"]
    if c.wpack == "ring":
        dev["wp"] = ops.pack_conv_weight_ring(w)
    elif c.wpack == "ring_dgrad":
        dev["wp"] = ops.pack_conv_weight_ring_dgrad(w)
    elif c.wpack == "s2_dgrad":
        dev["wp"], kt = ops.pack_conv_weight_s2_dgrad(w, {2: 1, 4: 3}[c.K])
        assert kt == c.K
    elif c.entry in ("s2", "dual") and c.K > 1:
        dev["wp"] = ops.pack_conv_weight_s2d(w, c.pad)
    else:
        dev["wp"] = ops.pack_conv_weight(w, c.dt)
    return dev


def _run(c, dev, monkeypatch, env=None):
    """One call of the case's op under the case's switches.  Returns (y, y2, stats)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    env = dict(c.env) if env is None else env
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if env == dict(c.env):
        assert R.expected_inst(c) == c.inst
    if c.kernel == "ring":
        assert ops.conv_ring_ok(c.B, c.H, c.W, c.Cx, c.C2, c.up, c.Cout, c.head_n), c.name
    stats = None if dev["stats0"] is None else dev["stats0"].clone()
    y2 = None
    if c.entry == "head":
        y = ops.conv3x3_head_nchw(dev["x"], dev["wp"], dev["scale"], dev["shift"], dev["head_w"], dev["head_b"],
                                  x2=dev["x2"], up=c.up, relu=c.relu)
    elif c.entry == "s2":
        y = ops.conv2d_s2_nhwc(dev["x"], dev["wp"], c.K, c.pad, dev["scale"], dev["shift"], dev["residual"], c.relu,
                               stats=stats)
    elif c.entry == "dual":
        y, y2 = ops.conv2d_s2_dual_nhwc(dev["x"], dev["wp"], dev["scale"], dev["shift"], c.split, relu=c.relu)
    else:
        y = ops.conv2d_nhwc(dev["x"], dev["wp"], (c.K, c.K), 1, c.pad, dev["scale"], dev["shift"], dev["residual"],
                            c.relu, dev["x2"], c.up, stats, c.dt)
    for k in env:
        monkeypatch.delenv(k)
    return y, y2, stats


def _assert_equal(c, got, want64, what):
    want = R.expected(c, want64)
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got.double() != want.double()).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ from the exact reference; first at %s: got %r want %r; all "
                             "differing positions span %s .. %s" % (what, bad.shape[0], got.numel(), i, float(got[i]),
                                                                    float(want[i]), bad.amin(0).tolist(), bad.amax(0).tolist()))


@pytest.mark.parametrize("c", R.EXACT_CASES, ids=_id)
def test_exact_case_equals_fp64(c, monkeypatch):
    """Integer / dyadic operands: every fp32 summation order gives the reference's bits (R._assert_exact)."""
    dev, ref = _device(c.name), R.reference(c.name)
    before = ops.N.lib().lss_conv2d_ring_timeouts()
    y, y2, stats = _run(c, dev, monkeypatch)
    _assert_equal(c, y, ref.out, "conv_fwd." + c.name)
    if y2 is not None:
        _assert_equal(c, y2, ref.out2, "conv_fwd." + c.name + ".y2")
    if stats is not None:
        R.check(stats, ref.stats, ref.stats_bound, "conv_fwd." + c.name + ".stats")
    assert ops.N.lib().lss_conv2d_ring_timeouts() == before, "a flag wait of the ring kernel hit its bound"


@pytest.mark.parametrize("c", R.DIRECT_REPEATS, ids=_id)
def test_exact_tile_case_on_the_direct_kernel(c, monkeypatch):
    """The same operands under LSS_CONV_DIRECT=1: conv_direct_kernel<bf16, plain | fused>."""
    env = {"LSS_CONV_DIRECT": "1"}
    assert R.tile_inst(c, env) == "direct<bf16,%s>" % ("fused" if c.up > 1 or c.C2 else "plain")
    y, _, _ = _run(c, _device(c.name), monkeypatch, env)
    _assert_equal(c, y, R.reference(c.name).out, "conv_fwd.direct." + c.name)


def _report(report, tag, emax, el2, bound, ref):
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    report(tag + ".bound_over_max", float(bound.max() / ref.abs().max()))


@pytest.mark.parametrize("c", R.BOUND_CASES, ids=_id)
def test_bound_case_against_fp64(c, report, monkeypatch):
    """Real-valued operands inside the derived elementwise bound; the measured ratios go on record."""
    dev, ref = _device(c.name), R.reference(c.name)
    assert ref.share <= R.AMBIGUOUS_CAP
    before = ops.N.lib().lss_conv2d_ring_timeouts()
    y, y2, stats = _run(c, dev, monkeypatch)
    tag = "conv_fwd." + c.name
    assert y.dtype == (torch.float32 if (c.head_n or c.dt == R.F32) else torch.bfloat16)
    _report(report, tag, *R.check(y, ref.out, ref.bound, tag), ref.bound, ref.out)
    if y2 is not None:
        _report(report, tag + ".y2", *R.check(y2, ref.out2, ref.bound2, tag + ".y2"), ref.bound2, ref.out2)
    if stats is not None:
        _report(report, tag + ".stats", *R.check(stats, ref.stats, ref.stats_bound, tag + ".stats"), ref.stats_bound,
                ref.stats)
    assert ops.N.lib().lss_conv2d_ring_timeouts() == before, "a flag wait of the ring kernel hit its bound"


def test_ring_switch_off_refuses_the_ring_plan(monkeypatch):
    """LSS_CONV_RING=0 is read on every call: ops.conv_ring_ok then says no for a shape the kernel takes."""
    c = R.BY_NAME["r_plain_one_chunk"]
    monkeypatch.delenv("LSS_CONV_RING", raising=False)
    assert ops.conv_ring_ok(c.B, c.H, c.W, c.Cx, c.C2, c.up, c.Cout, c.head_n)
    monkeypatch.setenv("LSS_CONV_RING", "0")
    assert not ops.conv_ring_ok(c.B, c.H, c.W, c.Cx, c.C2, c.up, c.Cout, c.head_n)
