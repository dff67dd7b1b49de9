"""The stem mode of the K-split one-pass kernel (csrc/conv_ks.hip: conv_ks_stem_kernel), host side only: which shapes
its plan takes, the size of its weight image, that every argument check answers before any HIP call, and that the header
and the binding table declare the same four entries."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lss_conv2d_ks_stem_ok", "lss_conv2d_ks_stem_packed_weight_bytes", "lss_conv2d_pack_weights_ks_stem",
           "lss_conv2d_ks_stem_fwd"]


@pytest.fixture(scope="module")
def lib():
    from lss2_multimodal_nu_amd import build_native, _native
    build_native.build(verbose=False)
    return _native.lib()


def test_plan_takes_the_benched_shape_and_refuses_the_rest(lib, monkeypatch):
    monkeypatch.delenv("LSS_CONV_KS", raising=False)
    ok = lib.lss_conv2d_ks_stem_ok
    assert ok(4, 200, 200, 64, 64) == 1       # the benched stem: 4 x 9 x 7 tiles of 12 x 16 = 252 workgroups
    assert ok(1, 200, 200, 64, 64) == 1       # batch 1: 63
    assert ok(4, 199, 197, 64, 64) == 1       # odd sizes: 100 x 99 outputs
    assert ok(2, 200, 200, 64, 128) == 1      # two 64-channel blocks: 252
    assert ok(4, 200, 200, 128, 64) == 0 and ok(4, 200, 200, 32, 64) == 0    # Cin != 64
    assert ok(4, 200, 200, 64, 96) == 0 and ok(4, 200, 200, 64, 32) == 0     # Cout % 64
    assert ok(32, 23, 31, 64, 64) == 1        # 12 x 16 outputs: one tile per image, 32 workgroups - the smallest
    assert ok(32, 21, 31, 64, 64) == 0        # 11 output rows: below the tile
    assert ok(32, 23, 29, 64, 64) == 0        # 15 output columns
    assert ok(31, 23, 31, 64, 64) == 0        # 31 workgroups
    assert ok(4, 192, 256, 64, 64) == 1       # 96 x 128 outputs: 4 x 8 x 8 = 256 workgroups - the largest grid
    assert ok(4, 194, 256, 64, 64) == 0       # 97 rows: 4 x 9 x 8 = 288, a second round
    assert ok(4, 200, 200, 64, 128) == 0      # 504
    assert ok(2, 400, 400, 64, 64) == 0       # the hires workload: 2 x 17 x 13 = 442
    assert ok(0, 200, 200, 64, 64) == 0 and ok(4, 0, 200, 64, 64) == 0
    monkeypatch.setenv("LSS_CONV_KS", "0")    # the A/B switch of the kernel family
    assert ok(4, 200, 200, 64, 64) == 0


def test_weight_image_size_and_argument_checks(lib, monkeypatch):
    monkeypatch.delenv("LSS_CONV_KS", raising=False)
    nb = lib.lss_conv2d_ks_stem_packed_weight_bytes
    assert nb(64, 64) == 64 * 64 * 49 * 2 and nb(128, 64) == 128 * 64 * 49 * 2
    assert nb(96, 64) == 0 and nb(64, 128) == 0 and nb(0, 64) == 0
    one = ctypes.c_void_p(16)
    odd = ctypes.c_void_p(24)
    fwd, pack = lib.lss_conv2d_ks_stem_fwd, lib.lss_conv2d_pack_weights_ks_stem
    assert fwd(None, one, None, None, one, 4, 200, 200, 64, 64, 1, None) == -1    # LSS_E_NULL
    assert fwd(one, None, None, None, one, 4, 200, 200, 64, 64, 1, None) == -1
    assert fwd(one, one, None, None, None, 4, 200, 200, 64, 64, 1, None) == -1
    assert fwd(one, one, None, None, one, 2, 400, 400, 64, 64, 1, None) == -2     # LSS_E_SHAPE
    assert fwd(one, one, None, None, one, 4, 200, 200, 128, 64, 1, None) == -2
    assert fwd(one, one, None, None, one, 4, 200, 200, 64, 64, 2, None) == -3     # LSS_E_LAYOUT
    assert fwd(one, one, None, None, odd, 4, 200, 200, 64, 64, 1, None) == -4     # LSS_E_ALIGN
    assert fwd(odd, one, None, None, one, 4, 200, 200, 64, 64, 1, None) == -4
    assert fwd(one, one, odd, None, one, 4, 200, 200, 64, 64, 1, None) == -4
    assert pack(None, 64, 64, one, None) == -1
    assert pack(one, 64, 64, None, None) == -1
    assert pack(one, 96, 64, one, None) == -2
    assert pack(one, 64, 128, one, None) == -2


def test_header_and_binding_table_agree():
    from lss2_multimodal_nu_amd import _native
    src = open(os.path.join(ROOT, "include", "lss_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lss_[a-z0-9_]+)\s*\(", src))
    for name in ENTRIES:
        assert name in declared and name in _native.SIGNATURES
    # argument counts of the declarations against the ctypes table
    for name in ENTRIES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m is not None
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_native.SIGNATURES[name][1])
