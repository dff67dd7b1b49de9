"""K10 (csrc/pointwise_grad.hip), the backward of a 1x1 conv, against a float64 einsum on the CPU of the same fp32
operands.  Bound: the project's rule for fp32-accumulated gradient kernels against fp64, rtol 2e-4,
atol 2e-5 * max|ref| (test_kernels_gpu.py, K7).

Cases: the full product of the listed values (3 layouts x 3 M x 5 K x 4 HW x 3 BN = 540) would spend minutes of float64
einsum per run, so the set below is a cover instead: every M, K, HW and BN value appears with every layout, every
(M, K) pair and every (HW, BN) pair appears at least once, and the largest and the smallest corner are both there.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import _native  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402

MS, KS, HWS, BNS = (41, 105, 128), (64, 256, 512, 768, 1024), (1, 44, 176, 189), (1, 24, 48)
LAYOUTS = ("nchw", "nhwc", "nhwc_bf16")


def _cases():
    """15 (M, K) pairs interleaved with 12 (HW, BN) pairs: 15 shapes, each (M, K) once, each (HW, BN) at least once."""
    mk = [(m, k) for k in KS for m in MS]
    hb = [(hw, bn) for hw in HWS for bn in BNS]
    out = [(mk[i][0], mk[i][1], hb[(5 * i) % 12][0], hb[(5 * i) % 12][1]) for i in range(15)]  # 5 coprime to 12
    out += [(128, 1024, 189, 48), (41, 64, 1, 1)]
    return sorted(set(out))


def _operands(M, K, HW, BN, layout, seed, off=0, wide=0):
    gen = torch.Generator().manual_seed(seed)
    gw = torch.randn(BN, M + wide, HW, generator=gen)
    x = torch.randn(BN, K, HW, generator=gen)
    w = torch.randn(M, K, generator=gen) / K ** 0.5
    if layout == "nhwc_bf16":
        x = x.bfloat16().float()  # the reference sees the bf16-rounded x widened exactly
    return gw, x, w


def _x_dev(x, layout):
    if layout == "nchw":
        return x.cuda()
    xr = x.permute(0, 2, 1).contiguous().cuda()
    return xr.bfloat16() if layout == "nhwc_bf16" else xr


def _reference(g, x, w):
    g64, x64, w64 = g.double(), x.double(), w.double()
    return (torch.einsum("mk,bmp->bkp", w64, g64), torch.einsum("bmp,bkp->mk", g64, x64), g64.sum((0, 2)))


def _close(got, ref, what):
    ref = ref.numpy()
    np.testing.assert_allclose(got.double().cpu().numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=what)


def _dx_ref_as(dx_ref, layout):
    return dx_ref if layout == "nchw" else dx_ref.permute(0, 2, 1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,K,HW,BN", _cases())
def test_against_float64(M, K, HW, BN, layout):
    g, x, w = _operands(M, K, HW, BN, layout, seed=M + K + HW + BN)
    dx_ref, dw_ref, db_ref = _reference(g, x, w)
    lay = "nchw" if layout == "nchw" else "nhwc"
    dx, dw, db = ops.pointwise_conv_bwd(g.cuda(), _x_dev(x, layout), w.cuda(), layout=lay)
    assert dw.shape == w.shape and db.shape == (M,)
    if layout == "nhwc_bf16":
        # dx is stored in x's dtype: one bf16 rounding (2^-9 relative) on top of the fp32 result
        assert dx.dtype == torch.bfloat16
        ref = _dx_ref_as(dx_ref, layout).numpy()
        np.testing.assert_allclose(dx.double().cpu().numpy(), ref, rtol=2e-4 + 2.0 ** -8,
                                   atol=2e-5 * np.abs(ref).max(), err_msg="dx")
    else:
        _close(dx, _dx_ref_as(dx_ref, layout), "dx")
    _close(dw, dw_ref, "dw")
    _close(db, db_ref, "db")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_offset_channel_range_of_wider_tensor(layout):
    """g = channels [41, 41 + 128) of a (BN, 41 + 128 + 3, HW) tensor, and its first 41 as a strided slice view."""
    M, K, HW, BN, off = 128, 256, 176, 24, 41
    gw, x, w = _operands(M, K, HW, BN, layout, seed=3, wide=off + 3)
    lay = "nchw" if layout == "nchw" else "nhwc"
    gd, xd = gw.cuda(), _x_dev(x, layout)
    dx_ref, dw_ref, db_ref = _reference(gw[:, off:off + M], x, w)
    dx, dw, db = ops.pointwise_conv_bwd(gd, xd, w.cuda(), layout=lay, g_ch_off=off, M=M)
    if layout != "nhwc_bf16":
        _close(dx, _dx_ref_as(dx_ref, layout), "dx")
    _close(dw, dw_ref, "dw")
    _close(db, db_ref, "db")
    view = gd[:, off:off + M]  # a slice view: same storage, read in place
    assert not view.is_contiguous()
    dx2, dw2, db2 = ops.pointwise_conv_bwd(view, xd, w.cuda(), layout=lay)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    w41 = w[:off].contiguous()
    dx_ref, dw_ref, db_ref = _reference(gw[:, :off], x, w41)
    dx3, dw3, db3 = ops.pointwise_conv_bwd(gd[:, :off], xd, w41.cuda(), layout=lay)
    _close(dw3, dw_ref, "dw41")
    _close(db3, db_ref, "db41")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("skip", ["dx", "dw", "db"])
def test_each_output_skipped(layout, skip):
    M, K, HW, BN = 105, 512, 44, 24
    g, x, w = _operands(M, K, HW, BN, layout, seed=11)
    lay = "nchw" if layout == "nchw" else "nhwc"
    args = (g.cuda(), _x_dev(x, layout), w.cuda())
    full = ops.pointwise_conv_bwd(*args, layout=lay)
    part = ops.pointwise_conv_bwd(*args, layout=lay, want_dx=skip != "dx", want_dw=skip != "dw", want_db=skip != "db")
    for name, a, b in zip(("dx", "dw", "db"), full, part):
        if name == skip:
            assert b is None
        else:
            assert torch.equal(a, b), name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_runs_bit_equal(layout):
    M, K, HW, BN = 105, 512, 176, 24
    g, x, w = _operands(M, K, HW, BN, layout, seed=5)
    lay = "nchw" if layout == "nchw" else "nhwc"
    args = (g.cuda(), _x_dev(x, layout), w.cuda())
    a = ops.pointwise_conv_bwd(*args, layout=lay)
    torch.empty(1 << 22, device="cuda").normal_()  # move the allocator: the workspace lands elsewhere
    b = ops.pointwise_conv_bwd(*args, layout=lay)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_refused_shapes_touch_nothing():
    L = _native.lib()
    assert L.lss_pointwise_conv_bwd_ok(24, 512, 105, 176) == 1
    for BN, K, M, HW in [(24, 96, 41, 176), (24, 1088, 41, 176), (24, 512, 193, 176), (24, 512, 41, 0), (0, 512, 41, 176)]:
        assert L.lss_pointwise_conv_bwd_ok(BN, K, M, HW) == 0
        assert L.lss_pointwise_conv_bwd_workspace_bytes(BN, K, M, HW) == 0
    BN, K, M, HW = 4, 96, 41, 44  # K % 64 != 0
    g = torch.randn(BN, M, HW, device="cuda")
    x = torch.randn(BN, K, HW, device="cuda")
    w = torch.randn(M, K, device="cuda")
    ws = torch.zeros(1 << 20, device="cuda")
    outs = [torch.full((BN, K, HW), 7.0, device="cuda"), torch.full((M, K), 7.0, device="cuda"),
            torch.full((M,), 7.0, device="cuda")]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lss_pointwise_conv_bwd(p(g), 0, M * HW, p(x), 0, p(w), BN, K, M, HW, p(ws), ws.numel() * 4, p(outs[0]),
                                  p(outs[1]), p(outs[2]), None)
    torch.cuda.synchronize()
    assert rc == -2  # LSS_E_SHAPE
    assert all(bool((o == 7.0).all()) for o in outs) and bool((ws == 0).all())
    with pytest.raises(ValueError):
        ops.pointwise_conv_bwd(g, x, w)


def test_inf_in_g_gives_nonfinite_dw():
    M, K, HW, BN = 41, 256, 176, 12
    g, x, w = _operands(M, K, HW, BN, "nchw", seed=9)
    g[5, 17, 100] = float("inf")
    dx, dw, db = ops.pointwise_conv_bwd(g.cuda(), x.cuda(), w.cuda())
    assert not bool(torch.isfinite(dw[17]).all())
    assert not bool(torch.isfinite(db[17]))
    assert not bool(torch.isfinite(dx[5, :, 100]).all())
    # and only there: the other rows / pixels are the clean run's
    g[5, 17, 100] = 0.0
    dx0, dw0, db0 = ops.pointwise_conv_bwd(g.cuda(), x.cuda(), w.cuda())
    keep = torch.ones(M, dtype=torch.bool, device="cuda")
    keep[17] = False
    assert torch.equal(dw[keep], dw0[keep]) and torch.equal(db[keep], db0[keep])
    dx[5, :, 100] = dx0[5, :, 100]
    assert torch.equal(dx, dx0)
