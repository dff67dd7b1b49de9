"""CPU-side checks of the deformable-attention entries (lss_deform_attn_fwd, lss_deform_attn_pts_fwd,
lss_deform_attn_bwd, lss_deform_attn_bwd_workspace_bytes) and of lss_add_pos_fwd: every argument check runs before any
HIP call, so the documented error codes come back without a GPU."""
import ctypes

import pytest

E_NULL, E_SHAPE, E_LAYOUT, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4, -5


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


def infer(L, value=A, layout=0, ol=A, tb=None, rx=A, ry=A, B=2, H=4, W=4, nh=8, npt=8, C=256, dt=0, out=A):
    return L.lss_deform_attn_fwd(value, layout, ol, tb, rx, ry, B, H, W, nh, npt, C, dt, out, None)


def test_inference_forward_argument_checks(L):
    for k in ("value", "ol", "rx", "ry", "out"):
        assert infer(L, **{k: None}) == E_NULL, k
    assert infer(L, nh=4) == E_SHAPE
    assert infer(L, npt=4) == E_SHAPE
    assert infer(L, C=128) == E_SHAPE
    for k in ("B", "H", "W"):
        assert infer(L, **{k: 0}) == E_SHAPE, k
        assert infer(L, **{k: -1}) == E_SHAPE, k
    assert infer(L, B=1 << 11, H=1 << 10, W=1 << 10) == E_SHAPE       # B*H*W = 2^31
    assert infer(L, B=2, H=1 << 15, W=1 << 15) == E_SHAPE
    for layout in (-1, 2):
        assert infer(L, layout=layout) == E_LAYOUT
    for dt in (-1, 2):
        assert infer(L, dt=dt) == E_LAYOUT
    for k in ("value", "ol", "out"):
        for off in (4, 8):
            assert infer(L, **{k: _p((1 << 20) + off)}) == E_ALIGN, (k, off)
    # token_bias is read with 16-B loads as well; a null token_bias is "no bias" and never an error of its own
    for off in (4, 8):
        assert infer(L, tb=_p((1 << 20) + off)) == E_ALIGN
        assert infer(L, tb=_p((1 << 20) + off), layout=1, dt=1) == E_ALIGN
    assert infer(L, tb=None, value=None) == E_NULL
    assert infer(L, tb=A, nh=4) == E_SHAPE           # an aligned bias passes its check: the next one answers


def add_pos(L, x=A, pos=A, B=2, T=16, C=256, dt=0, q=A):
    return L.lss_add_pos_fwd(x, pos, B, T, C, dt, q, None)


def test_add_pos_argument_checks(L):
    for k in ("x", "pos", "q"):
        assert add_pos(L, **{k: None}) == E_NULL, k
    assert add_pos(L, C=128) == E_SHAPE
    for k in ("B", "T"):
        assert add_pos(L, **{k: 0}) == E_SHAPE, k
        assert add_pos(L, **{k: -3}) == E_SHAPE, k
    assert add_pos(L, B=1 << 16, T=1 << 15) == E_SHAPE                # B*T = 2^31
    for dt in (-1, 2):
        assert add_pos(L, dt=dt) == E_LAYOUT
    for k in ("x", "pos", "q"):
        for off in (4, 8):
            assert add_pos(L, **{k: _p((1 << 20) + off)}) == E_ALIGN, (k, off)
