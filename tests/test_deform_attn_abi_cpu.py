"""CPU-side checks of the deformable-attention training entries (lss_deform_attn_pts_fwd, lss_deform_attn_bwd,
lss_deform_attn_bwd_workspace_bytes): every argument check runs before any HIP call, so the documented error codes
come back without a GPU."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -4, -5


@pytest.fixture(scope="module")
def L():
    from lss2_multimodal_nu_amd import _native, build_native
    build_native.build(verbose=False)
    return _native.lib()


def _p(addr):
    return ctypes.c_void_p(addr)


A = _p(1 << 20)  # a 16-B aligned (never dereferenced) address


def test_workspace_bytes_formula(L):
    for B, H, W in [(1, 1, 1), (2, 12, 12), (8, 200, 200), (3, 9, 14)]:
        assert L.lss_deform_attn_bwd_workspace_bytes(B, H, W) == H * W * (256 * 8 + 8 * 4) + 4 * B
    assert L.lss_deform_attn_bwd_workspace_bytes(0, 4, 4) == 0
    assert L.lss_deform_attn_bwd_workspace_bytes(1, -1, 4) == 0
    assert L.lss_deform_attn_bwd_workspace_bytes(1, 4, 0) == 0


def fwd(L, value=A, ol=A, ref=A, rstride=0, B=2, H=4, W=4, nh=8, npt=8, C=256, out=A):
    return L.lss_deform_attn_pts_fwd(value, ol, ref, rstride, B, H, W, nh, npt, C, out, None)


def test_forward_argument_checks(L):
    assert fwd(L, value=None) == E_NULL
    assert fwd(L, ol=None) == E_NULL
    assert fwd(L, ref=None) == E_NULL
    assert fwd(L, out=None) == E_NULL
    assert fwd(L, nh=4) == E_SHAPE
    assert fwd(L, npt=4) == E_SHAPE
    assert fwd(L, C=128) == E_SHAPE
    assert fwd(L, B=0) == E_SHAPE
    assert fwd(L, H=-1) == E_SHAPE
    assert fwd(L, rstride=-2) == E_SHAPE
    assert fwd(L, value=_p((1 << 20) + 4)) == E_ALIGN
    assert fwd(L, ol=_p((1 << 20) + 8)) == E_ALIGN
    assert fwd(L, out=_p((1 << 20) + 4)) == E_ALIGN
    assert fwd(L, ref=_p((1 << 20) + 4)) == E_ALIGN  # ref_pts needs 8 B
    assert fwd(L, rstride=3) == E_ALIGN               # odd sample stride breaks the 8-B point loads


def bwd(L, value=A, ol=A, ref=A, rstride=32, dout=A, B=2, H=4, W=4, nh=8, npt=8, C=256, ws=A, wsb=None,
        dv=A, dol=A):
    if wsb is None:
        wsb = L.lss_deform_attn_bwd_workspace_bytes(B, H, W) if B > 0 and H > 0 and W > 0 else 0
    return L.lss_deform_attn_bwd(value, ol, ref, rstride, dout, B, H, W, nh, npt, C, ws, wsb, dv, dol, None)


def test_backward_argument_checks(L):
    for k in ("value", "ol", "ref", "dout", "ws", "dv", "dol"):
        assert bwd(L, **{k: None}) == E_NULL, k
    assert bwd(L, nh=16) == E_SHAPE
    assert bwd(L, npt=4) == E_SHAPE
    assert bwd(L, C=512) == E_SHAPE
    assert bwd(L, W=0) == E_SHAPE
    assert bwd(L, rstride=-32) == E_SHAPE
    for k in ("value", "ol", "dout", "ws", "dv", "dol"):
        assert bwd(L, **{k: _p((1 << 20) + 4)}) == E_ALIGN, k
    assert bwd(L, ref=_p((1 << 20) + 4)) == E_ALIGN
    assert bwd(L, rstride=31) == E_ALIGN
    need = L.lss_deform_attn_bwd_workspace_bytes(2, 4, 4)
    assert bwd(L, wsb=need - 1) == E_WORKSPACE
