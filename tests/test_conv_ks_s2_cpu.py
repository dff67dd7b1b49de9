"""The stride-2 mode of the K-split one-pass kernel (csrc/conv_ks.hip), host side only: which shapes its plan takes,
the size of its weight image, and that every argument check answers before any HIP call."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from lss2_multimodal_nu_amd import build_native, _native
    build_native.build(verbose=False)
    return _native.lib()


def test_plan_takes_the_benched_shapes_and_refuses_the_rest(lib, monkeypatch):
    monkeypatch.delenv("LSS_CONV_KS", raising=False)
    ok = lib.lss_conv2d_ks_s2_dual_ok
    assert ok(4, 100, 100, 64, 128) == 1      # layer2.0: 4 x 27 x 2 = 216 workgroups
    assert ok(4, 50, 50, 128, 256) == 1       # layer3.0: 4 x 14 x 4 = 224
    assert ok(4, 99, 97, 64, 128) == 1 and ok(4, 53, 51, 128, 256) == 1   # odd sizes
    assert ok(4, 200, 200, 64, 128) == 0      # hires: patch too wide for LDS
    assert ok(4, 128, 128, 64, 128) == 0      # 64 outputs per row: 7 x 129 positions x 128 B > 112 KiB
    assert ok(4, 126, 126, 64, 128) == 1      # 63: the widest
    assert ok(4, 94, 94, 64, 128) == 0        # 47 outputs per row: a 96-pixel block could span four rows
    assert ok(4, 64, 64, 128, 256) == 0 and ok(4, 46, 46, 128, 256) == 0
    assert ok(4, 100, 100, 64, 96) == 0       # Cout % 64
    assert ok(4, 25, 25, 256, 512) == 0       # Cin 256 is not a case
    assert ok(1, 50, 50, 128, 256) == 0       # 56 workgroups
    assert ok(16, 100, 100, 64, 128) == 0     # 864 workgroups
    monkeypatch.setenv("LSS_CONV_KS", "0")    # the A/B switch of the kernel family
    assert ok(4, 100, 100, 64, 128) == 0


def test_weight_image_size_and_argument_checks(lib):
    nb = lib.lss_conv2d_ks_s2_dual_packed_weight_bytes
    assert nb(128, 64) == 128 * 64 * 10 * 2 and nb(256, 128) == 256 * 128 * 10 * 2
    assert nb(96, 64) == 0 and nb(128, 256) == 0 and nb(0, 64) == 0
    one = ctypes.c_void_p(16)
    odd = ctypes.c_void_p(24)
    fwd, pack = lib.lss_conv2d_ks_s2_dual_fwd, lib.lss_conv2d_pack_weights_ks_s2_dual
    assert fwd(None, one, None, None, one, one, 4, 100, 100, 64, 128, 1, None) == -1
    assert fwd(one, one, None, None, one, None, 4, 100, 100, 64, 128, 1, None) == -1
    assert fwd(one, one, None, None, one, one, 4, 200, 200, 64, 128, 1, None) == -2
    assert fwd(one, one, None, None, one, one, 4, 100, 100, 64, 128, 2, None) == -3
    assert fwd(one, one, None, None, odd, one, 4, 100, 100, 64, 128, 1, None) == -4
    assert pack(one, None, 128, 64, one, None) == -1
    assert pack(one, one, 128, 96, one, None) == -2
