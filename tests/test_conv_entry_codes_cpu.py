"""The tile-kernel conv entries of csrc/conv_mfma.hip (lss_conv2d_fwd, _s2_fwd, _s2_dual_fwd, _head_fwd, _sequence),
host side only: which code every refused call gets, and that the answer comes before any HIP call (fake aligned
pointers, no GPU).  The order of the checks is part of it: a call wrong in two ways gets the code of the first check."""
import ctypes

import pytest

P = ctypes.c_void_p(4096)   # a fake, aligned, never dereferenced device pointer
NULL, SHAPE, LAYOUT = -1, -2, -3
W_RING, W_KS = 64, 128
SWITCHES = ("LSS_CONV_WT", "LSS_CONV_DIRECT", "LSS_CONV_RT", "LSS_CONV_KC", "LSS_CONV_STAMPS", "LSS_CONV_KS",
            "LSS_CONV_RING")


@pytest.fixture(scope="module")
def lib():
    from lss2_multimodal_nu_amd import build_native, _native
    build_native.build(verbose=False)
    return _native.lib()


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _fwd(lib, **kw):
    a = dict(x=P, x2=None, w=P, scale=None, shift=None, residual=None, y=P, stats=None, B=1, H=16, W=16, Cx=64, C2=0,
             up=1, Cout=64, KH=3, KW=3, stride=1, pad=1, relu=0, dt=1)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.lss_conv2d_fwd(a["x"], a["x2"], a["w"], a["scale"], a["shift"], a["residual"], a["y"], a["stats"],
                              a["B"], a["H"], a["W"], a["Cx"], a["C2"], a["up"], a["Cout"], a["KH"], a["KW"],
                              a["stride"], a["pad"], a["relu"], a["dt"], None)


def _s2(lib, **kw):
    a = dict(x=P, w=P, scale=None, shift=None, residual=None, y=P, stats=None, B=1, H=16, W=16, Cx=64, Cout=64, K=3,
             pad=1, relu=0)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.lss_conv2d_s2_fwd(a["x"], a["w"], a["scale"], a["shift"], a["residual"], a["y"], a["stats"], a["B"],
                                 a["H"], a["W"], a["Cx"], a["Cout"], a["K"], a["pad"], a["relu"], None)


def _dual(lib, **kw):
    a = dict(x=P, w=P, scale=None, shift=None, y=P, y2=P, B=1, H=16, W=16, Cx=64, Cout=256, split=128, K=3, pad=1,
             relu=0)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.lss_conv2d_s2_dual_fwd(a["x"], a["w"], a["scale"], a["shift"], a["y"], a["y2"], a["B"], a["H"], a["W"],
                                      a["Cx"], a["Cout"], a["split"], a["K"], a["pad"], a["relu"], None)


def _head(lib, **kw):
    a = dict(x=P, x2=None, w=P, scale=None, shift=None, head_w=P, head_b=P, out=P, B=1, H=16, W=16, Cx=64, C2=0, up=1,
             Cout=128, head_n=4, relu=1)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.lss_conv2d_head_fwd(a["x"], a["x2"], a["w"], a["scale"], a["shift"], a["head_w"], a["head_b"], a["out"],
                                   a["B"], a["H"], a["W"], a["Cx"], a["C2"], a["up"], a["Cout"], a["head_n"], a["relu"],
                                   None)


def test_conv2d_fwd_codes(lib):
    for name in ("x", "w", "y"):
        assert _fwd(lib, **{name: None}) == NULL
    assert _fwd(lib, x=None, B=0) == NULL                       # pointers before sizes
    for name in ("B", "H", "Cx", "Cout", "KH", "stride", "up"):
        assert _fwd(lib, **{name: 0}) == SHAPE, name
    assert _fwd(lib, pad=-1) == SHAPE
    assert _fwd(lib, C2=-1) == SHAPE
    assert _fwd(lib, dt=2) == LAYOUT
    assert _fwd(lib, dt=2, C2=64) == LAYOUT                     # the dtype before the skip tensor's pointer
    assert _fwd(lib, C2=64) == NULL
    # KS-packed weights: the K-split kernel or nothing
    assert _fwd(lib, relu=W_KS, stride=2) == SHAPE
    assert _fwd(lib, relu=W_KS, stats=P) == SHAPE
    assert _fwd(lib, relu=W_KS | 2) == SHAPE
    assert _fwd(lib, relu=W_KS, C2=64, x2=P) == SHAPE
    assert _fwd(lib, relu=W_KS, dt=0) == SHAPE
    # ring-packed weights: the ring kernel or nothing
    assert _fwd(lib, relu=W_RING, residual=P) == SHAPE
    assert _fwd(lib, relu=W_RING, stats=P) == SHAPE
    assert _fwd(lib, relu=W_RING | 2) == SHAPE
    assert _fwd(lib, relu=W_RING, KH=1, KW=1) == SHAPE
    # K blocks
    assert _fwd(lib, Cx=48) == SHAPE
    assert _fwd(lib, up=2, Cx=32) == SHAPE
    assert _fwd(lib, C2=32, x2=P) == SHAPE
    assert _fwd(lib, dt=0, Cx=12) == SHAPE
    # the shared geometry: no output pixel; 2^31 of them
    assert _fwd(lib, H=1, W=1, pad=0) == SHAPE
    assert _fwd(lib, B=1 << 15, H=256, W=256) == SHAPE
    for relu in (3, 4, 8, 256):
        assert _fwd(lib, relu=relu) == LAYOUT, relu


def test_conv2d_s2_codes(lib):
    for name in ("x", "w", "y"):
        assert _s2(lib, **{name: None}) == NULL
    assert _s2(lib, B=0) == SHAPE
    assert _s2(lib, Cout=0) == SHAPE
    for K, pad in ((3, 0), (5, 2), (1, 1)):
        assert _s2(lib, K=K, pad=pad) == SHAPE, (K, pad)
    assert _s2(lib, Cx=32) == SHAPE
    assert _s2(lib, B=1 << 15, H=512, W=512) == SHAPE           # 2^31 output pixels


def test_conv2d_s2_dual_codes(lib):
    assert _dual(lib, y2=None) == NULL
    assert _dual(lib, y2=None, x=None, split=0) == NULL         # y2 before everything else
    for split in (0, 64, 256):
        assert _dual(lib, split=split) == SHAPE, split
    assert _dual(lib, Cout=132) == SHAPE
    assert _dual(lib, x=None) == NULL
    assert _dual(lib, K=5) == SHAPE


def test_conv2d_head_codes(lib):
    for name in ("x", "w", "head_w", "head_b", "out"):
        assert _head(lib, **{name: None}) == NULL, name
    for name in ("B", "up", "head_n"):
        assert _head(lib, **{name: 0}) == SHAPE, name
    assert _head(lib, relu=W_RING | 2) == SHAPE
    assert _head(lib, relu=W_RING | 1, C2=64) == NULL
    assert _head(lib, Cout=96) == SHAPE
    assert _head(lib, C2=-64) == SHAPE
    assert _head(lib, Cx=32) == SHAPE
    assert _head(lib, C2=32) == SHAPE                           # the K block before the skip tensor's pointer
    assert _head(lib, head_n=65) == SHAPE
    assert _head(lib, Cout=64, up=2) == SHAPE
    assert _head(lib, Cout=64, C2=64, x2=P) == SHAPE
    assert _head(lib, C2=64) == NULL


def test_conv2d_sequence_codes(lib):
    from lss2_multimodal_nu_amd import _native
    seq = lib.lss_conv2d_sequence
    one = _native.ConvLaunch()
    assert seq(None, 1, None) == NULL
    assert seq(ctypes.byref(one), -1, None) == SHAPE
    assert seq(ctypes.byref(one), 0, None) == 0
    assert seq(ctypes.byref(_native.ConvLaunch(kind=6)), 1, None) == LAYOUT
    for kind in range(6):
        assert seq(ctypes.byref(_native.ConvLaunch(kind=kind)), 1, None) == NULL, kind
    bad_k = _native.ConvLaunch(kind=1, x=P, w=P, y=P, B=1, H=16, W=16, Cx=64, Cout=64, KH=5, KW=5, stride=2, pad=2)
    assert seq(ctypes.byref(bad_k), 1, None) == SHAPE
    # a refused launch ends the list: the valid-looking second entry is never reached
    two = (_native.ConvLaunch * 2)(_native.ConvLaunch(kind=6), bad_k)
    assert seq(two, 2, None) == LAYOUT
