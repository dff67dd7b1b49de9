"""The vovnet depth-head kernels alone against fp64: K2v (`ops.camencode_v2`, every LSS_V2_CASE instantiation x hidden
dtype x math mode x softmax on / off), the forward of `_HeadProjFn`, the fusion tail (`ops.depth_fuse_softmax`) and the
K-block paths of K2 (`ops.depthnet_softmax`) that tests/test_kernels_gpu.py does not reach.

References, cases and bounds: tests/depth_head_ref.py.  Every bound is DERIVED there (fp32 accumulation of the operands
the kernel multiplies, rounded to bf16 first in bf16 math); nothing is taken from a kernel.  Every measured error is
`report`ed."""
import ctypes
import functools

import pytest
import torch

import depth_head_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import _native as N  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from lss2_multimodal_nu_amd.model_vovnet_transformer import _HeadProjFn  # noqa: E402

HIDDEN = {"hidden_f32": torch.float32, "hidden_bf16": torch.bfloat16}
BY_NAME = {c.name: c for c in R.V2_CASES}
E_SHAPE = -2
_id = lambda c: c.name  # noqa: E731


def test_abi_codes():
    assert (ops.DT_F32, ops.DT_BF16) == (R.F32, R.BF16)


@functools.lru_cache(maxsize=None)
def _v2_inputs(name, hkey):
    return R.make_v2_inputs(BY_NAME[name], HIDDEN[hkey])


@functools.lru_cache(maxsize=None)
def _v2_ref(name, hkey, math):
    """Computed once per (case, hidden dtype, math mode), shared by every test, never written to."""
    return R.ref_camencode_v2(*_v2_inputs(name, hkey), True, math)


@functools.lru_cache(maxsize=None)
def _v2_dev(name, hkey):
    return tuple(None if t is None else t.cuda() for t in _v2_inputs(name, hkey))


def _run_v2(name, hkey, softmax, math):
    c = BY_NAME[name]
    hidden, wd, bd, c3, wf, bf = _v2_dev(name, hkey)
    return ops.camencode_v2(hidden, wd, bd, c.D, c3, wf, bf, softmax=softmax, math=math)


def _v2_params():
    return [pytest.param(c.name, hkey, math, sm, id="%s-%s-math_%s-%s" % (c.name, hkey, R.MATH_NAME[math],
                                                                          "softmax" if sm else "logits"))
            for c in R.V2_CASES for hkey in HIDDEN for math in R.v2_modes(c) for sm in (True, False)]


@pytest.mark.parametrize("name,hkey,math,softmax", _v2_params())
def test_camencode_v2_against_fp64(name, hkey, math, softmax, report):
    c = BY_NAME[name]
    ref = _v2_ref(name, hkey, math)
    depth, feat = _run_v2(name, hkey, softmax, math)
    tag = "depth_heads.k2v.%s.%s.math_%s.%s" % (name, hkey, R.MATH_NAME[math], "prob" if softmax else "logits")
    assert depth.shape == (c.BN, c.D, c.fH, c.fW) and depth.dtype == torch.float32
    want, bound = (ref.prob, ref.bound_prob) if softmax else (ref.logits, ref.bound_logits)
    emax, el2 = R.check(depth, want, bound, tag)
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    report(tag + ".bound_over_max", float(bound.max() / want.abs().max()))
    if softmax:
        s = depth.double().sum(1).cpu()
        assert float((s - 1).abs().max()) <= R.sum_to_one_bound(c.D)
        if c.D == 1:
            assert bool((depth == 1.0).all())
    if c.C == 0:
        assert feat is None
    else:
        assert feat.shape == (c.BN, c.fH, c.fW, c.C) and feat.dtype == torch.float32
        fmax, fl2 = R.check(feat.reshape(c.BN, c.fH * c.fW, c.C), ref.feat, ref.bound_feat, tag + ".feat")
        report(tag + ".feat.max", fmax)
        report(tag + ".feat.l2", fl2)
        report(tag + ".feat.bound_over_max", float(ref.bound_feat.max() / ref.feat.abs().max()))


@pytest.mark.parametrize("c", R.V2_CASES, ids=_id)
@pytest.mark.parametrize("hkey", list(HIDDEN))
def test_camencode_v2_default_math(c, hkey):
    """math=None: the hidden map's own precision when the shapes allow (bf16 hidden, Cd and Cf multiples of 128)."""
    want = R.default_math(c, HIDDEN[hkey])
    d0, f0 = _run_v2(c.name, hkey, False, None)
    d1, f1 = _run_v2(c.name, hkey, False, want)
    assert torch.equal(d0, d1) and (f0 is None) == (c.C == 0) and (c.C == 0 or torch.equal(f0, f1))
    other = [m for m in R.v2_modes(c) if m != want]
    if other and c.Cd >= 128 and c.D > 1:   # the other mode multiplies other operands: it cannot give the same bits
        d2, _ = _run_v2(c.name, hkey, False, other[0])
        assert not torch.equal(d0, d2)


def _p(t, offset_floats=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


def _call_v2(c_like, dev, dt, softmax, math, depth_ptr, feat_ptr):
    BN, fH, fW, Cd, Cf, D, C = c_like
    hidden, wd, bd, c3, wf, bf = dev
    return N.lib().lss_camencode_v2_fwd(_p(hidden), dt, _p(wd), _p(bd), Cd, _p(c3), _p(wf), _p(bf), Cf, BN, fH * fW, D, C,
                                        1 if softmax else 0, math, depth_ptr, feat_ptr, N.stream())


@pytest.mark.parametrize("what,D,C,Cd,Cf,math", R.V2_REFUSED, ids=[r[0] for r in R.V2_REFUSED])
def test_camencode_v2_refused_shapes_touch_nothing(what, D, C, Cd, Cf, math):
    BN, fH, fW = 1, 3, 3
    gen = torch.Generator().manual_seed(1)
    hidden = torch.randn(BN, fH, fW, Cd, generator=gen).cuda()
    wd, bd = torch.randn(D, Cd, generator=gen).cuda(), torch.randn(D, generator=gen).cuda()
    c3 = torch.randn(BN, Cf, fH, fW, generator=gen).cuda()
    wf, bf = torch.randn(C, Cf, generator=gen).cuda(), torch.randn(C, generator=gen).cuda()
    # room for a whole 16-pixel tile of 16-row tiles beyond what the shape needs
    depth = torch.full((BN * 16 * ((D + 15) // 16) * 16 + 64,), 7.0, device="cuda")
    feat = torch.full((BN * 16 * 16 * ((C + 15) // 16) + 64,), 7.0, device="cuda")
    for dt, h in ((ops.DT_F32, hidden), (ops.DT_BF16, hidden.bfloat16())):
        rc = _call_v2((BN, fH, fW, Cd, Cf, D, C), (h, wd, bd, c3, wf, bf), dt, True, math, _p(depth), _p(feat))
        torch.cuda.synchronize()
        assert rc == E_SHAPE, (what, rc)
        assert bool((depth == 7.0).all()) and bool((feat == 7.0).all())
        with pytest.raises(ValueError):
            N.check(rc, "lss_camencode_v2_fwd")
        with pytest.raises(ValueError):
            ops.camencode_v2(h, wd, bd, D, c3, wf, bf, math=math)


PARTIAL = [c for c in R.V2_CASES if (c.fH * c.fW) % 16]


@pytest.mark.parametrize("c", PARTIAL, ids=_id)
@pytest.mark.parametrize("hkey", list(HIDDEN))
def test_camencode_v2_no_stray_writes(c, hkey):
    """depth and feat inside larger buffers, 64 sentinel floats on either side: the sentinels survive, every interior
    element is written (NaN pre-fill), and the interior is what the allocating call returns."""
    assert {"3_8_production_k", "3_4", "4_0"} <= {x.name for x in PARTIAL}
    dev = _v2_dev(c.name, hkey)
    dt = ops.DT_F32 if HIDDEN[hkey] == torch.float32 else ops.DT_BF16
    nd, nf = c.BN * c.D * c.fH * c.fW, c.BN * c.fH * c.fW * c.C
    for math in R.v2_modes(c):
        for softmax in (True, False):
            bufs = []
            for n in (nd, nf):
                b = torch.full((64 + n + 64,), float("nan"), device="cuda")
                b[:64] = 7.0
                b[64 + n:] = 7.0
                bufs.append(b)
            rc = _call_v2(c[1:], dev, dt, softmax, math, _p(bufs[0], 64), _p(bufs[1], 64) if c.C else None)
            torch.cuda.synchronize()
            assert rc == 0
            for b, n in zip(bufs, (nd, nf)):
                assert bool((b[:64] == 7.0).all()) and bool((b[64 + n:] == 7.0).all())
            assert bool(torch.isfinite(bufs[0][64:64 + nd]).all())
            depth, feat = _run_v2(c.name, hkey, softmax, math)
            assert torch.equal(bufs[0][64:64 + nd], depth.reshape(-1))
            if c.C:
                assert bool(torch.isfinite(bufs[1][64:64 + nf]).all())
                assert torch.equal(bufs[1][64:64 + nf], feat.reshape(-1))
            else:
                assert bool(torch.isnan(bufs[1][64:64 + nf]).all())


@pytest.mark.parametrize("math", [R.F32, R.BF16], ids=["math_f32", "math_bf16"])
@pytest.mark.parametrize("hkey", list(HIDDEN))
@pytest.mark.parametrize("softmax", [True, False], ids=["softmax", "logits"])
def test_camencode_v2_pixel_independence(math, hkey, softmax):
    """A NaN in one hidden channel of one pixel and a +inf in one c3 channel of another change those two pixels'
    outputs and nothing else."""
    c = BY_NAME["3_8_production_k"]
    hidden, wd, bd, c3, wf, bf = _v2_dev(c.name, hkey)
    clean_d, clean_f = _run_v2(c.name, hkey, softmax, math)
    (b0, h0, w0), (b1, h1, w1) = (1, 4, 6), (0, 2, 1)   # the last pixel of the partial tile, and one in a full tile
    hidden2, c32 = hidden.clone(), c3.clone()
    hidden2[b0, h0, w0, 131] = float("nan")
    c32[b1, 517, h1, w1] = float("inf")
    d, f = ops.camencode_v2(hidden2, wd, bd, c.D, c32, wf, bf, softmax=softmax, math=math)
    assert bool(torch.isnan(d[b0, :, h0, w0]).all())
    assert not bool(torch.isfinite(f[b1, h1, w1]).all())
    # the NaN pixel's context rows and the inf pixel's depth column come from the untouched operand
    assert torch.equal(f[b0, h0, w0], clean_f[b0, h0, w0]) and torch.equal(d[b1, :, h1, w1], clean_d[b1, :, h1, w1])
    d, f = d.clone(), f.clone()
    d[b0, :, h0, w0] = clean_d[b0, :, h0, w0]
    f[b1, h1, w1] = clean_f[b1, h1, w1]
    assert torch.equal(d, clean_d) and torch.equal(f, clean_f)


@pytest.mark.parametrize("math", [R.F32, R.BF16], ids=["math_f32", "math_bf16"])
@pytest.mark.parametrize("hkey", list(HIDDEN))
def test_camencode_v2_two_runs_bit_equal(math, hkey):
    a = _run_v2("3_8_production_k", hkey, True, math)
    torch.empty(1 << 20, device="cuda").normal_()   # move the allocator: the outputs land elsewhere
    b = _run_v2("3_8_production_k", hkey, True, math)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("with_c3", [True, False], ids=["with_c3", "without_c3"])
def test_head_proj_forward(with_c3, report):
    """`_HeadProjFn.forward` on an NCHW fp32 hidden map = K2v without softmax in fp32 math, bit for bit, and within the
    bound of the reference."""
    c = BY_NAME["3_8_production_k"]
    hidden, wd, bd, c3, wf, bf = _v2_dev(c.name, "hidden_f32")
    nchw = hidden.permute(0, 3, 1, 2).contiguous()
    args = (c3, wf.view(c.C, c.Cf, 1, 1), bf) if with_c3 else (None, None, None)
    with torch.no_grad():
        out = _HeadProjFn.apply(nchw, wd.view(c.D, c.Cd, 1, 1), bd, *args)
    logits, feat = out if with_c3 else (out, None)
    d, f = ops.camencode_v2(hidden, wd, bd, c.D, *((c3, wf, bf) if with_c3 else (None, None, None)), softmax=False,
                            math=ops.DT_F32)
    assert torch.equal(logits, d) and (f is None) == (feat is None) and (f is None or torch.equal(feat, f))
    ref = _v2_ref(c.name, "hidden_f32", R.F32)
    tag = "depth_heads.head_proj.%s" % ("with_c3" if with_c3 else "without_c3")
    emax, el2 = R.check(logits, ref.logits, ref.bound_logits, tag)
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    if with_c3:
        assert feat.shape == (c.BN, c.fH, c.fW, c.C)
        fmax, fl2 = R.check(feat.reshape(c.BN, -1, c.C), ref.feat, ref.bound_feat, tag + ".feat")
        report(tag + ".feat.max", fmax)
        report(tag + ".feat.l2", fl2)


# ----------------------------------------------------------------------------------------------------------------------
# the fusion tail
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fuse(name):
    c = next(x for x in R.FUSE_CASES if x.name == name)
    ins = R.make_fuse_inputs(c)
    return c, ins, R.ref_depth_fuse_softmax(*ins)


@pytest.mark.parametrize("c", R.FUSE_CASES, ids=_id)
def test_depth_fuse_softmax_against_fp64(c, report):
    _, ins, ref = _fuse(c.name)
    dev = [t.cuda() for t in ins]
    got = ops.depth_fuse_softmax(*dev)
    assert got.shape == (c.BN, c.D, c.H, c.W) and got.dtype == torch.float32
    tag = "depth_heads.fuse." + c.name
    emax, el2 = R.check(got, ref.prob, ref.bound_prob, tag)
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    report(tag + ".bound_over_max", float(ref.bound_prob.max() / ref.prob.max()))
    assert float((got.double().sum(1).cpu() - 1).abs().max()) <= R.sum_to_one_bound(c.D)
    # the clamped h1 / w1 path on its own slice, so that a failure names it
    R.check(got[:, :, -2:, :], ref.prob[:, :, -2:, :], ref.bound_prob[:, :, -2:, :], tag + ".last_two_rows")
    R.check(got[:, :, :, -2:], ref.prob[:, :, :, -2:], ref.bound_prob[:, :, :, -2:], tag + ".last_two_columns")
    if c.shift is not None:
        assert bool((got == torch.tensor(1.0) / torch.tensor(float(c.D))).all())   # expf(0) / D, correctly rounded
    if c.D == 1:
        assert bool((got == 1.0).all())
    again = ops.depth_fuse_softmax(*dev)
    assert torch.equal(got, again)


def test_depth_fuse_softmax_refusals():
    gen = torch.Generator().manual_seed(2)
    mk = lambda *s: torch.randn(*s, generator=gen).cuda()  # noqa: E731
    D = 65
    with pytest.raises(ValueError):
        ops.depth_fuse_softmax(mk(1, D, 2, 2), mk(1, D, 1, 1), mk(D, 2 * D), mk(D), mk(D))
    out = torch.full((1 * D * 2 * 2,), 7.0, device="cuda")
    ins = [mk(1, D, 2, 2), mk(1, D, 1, 1), mk(D, 2 * D), mk(D), mk(D)]
    rc = N.lib().lss_depth_fuse_softmax_fwd(*[_p(t) for t in ins], 1, D, 2, 2, 1, 1, _p(out), N.stream())
    torch.cuda.synchronize()
    assert rc == E_SHAPE and bool((out == 7.0).all())
    D = 5
    for d4 in (mk(3, D, 2, 2), mk(2, D + 1, 2, 2)):
        with pytest.raises(ValueError):
            ops.depth_fuse_softmax(mk(2, D, 4, 4), d4, mk(D, 2 * D), mk(D), mk(D))


# ----------------------------------------------------------------------------------------------------------------------
# K2: the K-block paths tests/test_kernels_gpu.py::test_k2_depthnet_softmax leaves out
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.K2_CASES, ids=_id)
def test_k2_depthnet_softmax_against_fp64(c, report):
    """fp32 math with one and with three 16-deep K blocks per wave (the odd tail of the pipelined loop); bf16 math
    against the rounded-operand reference."""
    x, w, b = R.make_k2_inputs(c)
    ref = R.ref_depthnet_softmax(x, w, b, c.D, c.C, c.math)
    dev = (x.cuda(), w.cuda(), b.cuda())
    depth, feat = ops.depthnet_softmax(*dev, c.D, c.C, c.math)
    assert depth.shape == (c.BN, c.D, c.fH, c.fW) and feat.shape == (c.BN, c.fH, c.fW, c.C)
    tag = "depth_heads.k2." + c.name
    emax, el2 = R.check(depth, ref.prob, ref.bound_prob, tag)
    fmax, fl2 = R.check(feat.reshape(c.BN, -1, c.C), ref.feat, ref.bound_feat, tag + ".feat")
    for k, v in ((".max", emax), (".l2", el2), (".feat.max", fmax), (".feat.l2", fl2),
                 (".bound_over_max", float(ref.bound_prob.max() / ref.prob.max())),
                 (".feat.bound_over_max", float(ref.bound_feat.max() / ref.feat.abs().max()))):
        report(tag + k, v)
    assert float((depth.double().sum(1).cpu() - 1).abs().max()) <= R.sum_to_one_bound(c.D)
    d2, f2 = ops.depthnet_softmax(*dev, c.D, c.C, c.math)
    assert torch.equal(depth, d2) and torch.equal(feat, f2)
