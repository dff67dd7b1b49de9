"""CPU-side checks of the native library: it builds for gfx950, loads without a
GPU, and exports exactly the symbols include/lss_hip.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "lss_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lss_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built():
    from lss2_multimodal_nu_amd import build_native
    return build_native.build(verbose=False)


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built)
    syms = header_symbols()
    assert len(syms) >= 14
    for s in syms:
        assert hasattr(lib, s), "missing export " + s


def test_binding_table_matches_header(built):
    from lss2_multimodal_nu_amd import _native
    assert sorted(_native.SIGNATURES) == header_symbols()
    L = _native.lib()
    assert L.lss_abi_version() == 1
    assert b"NULL" in L.lss_error_string(-1)


def test_argument_checks_without_gpu(built):
    """Argument validation happens before any HIP call, so it is testable here."""
    from lss2_multimodal_nu_amd import _native
    L = _native.lib()
    assert L.lss_points_to_voxels(None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 1, 1, 1, None, None, None, None) == -1
    assert L.lss_conv2d_packed_weight_bytes(4, 128, 1, 1, 1) == 4 * 128 * 2
    one = ctypes.c_void_p(16)
    assert L.lss_lift_splat_fwd(one, one, one, 1, 1, 1, 1, 1, 48, 1, 1, 1, one, 0, None) == -2  # C not 64/128
    assert L.lss_lift_splat_fwd(one, one, one, 1, 1, 1, 1, 1, 64, 1, 1, 1, one, 7, None) == -3  # bad layout
    assert L.lss_depthnet_softmax_fwd(one, one, one, 1, 100, 4, 4, 4, one, one, 0, None) == -2  # Cin % 64

    def desc(**fields):  # x == NULL form, every pointer it needs set, every size 1
        d = _native.LiftSplatDesc()
        for n in ("frustum", "inv_post_rots", "post_trans", "combine", "trans", "dx", "bx", "voxel", "vox_count",
                  "vox_list", "entries", "cursor", "depth", "feat", "bev"):
            setattr(d, n, one)
        d.B = d.N = d.D = d.fH = d.fW = d.X = d.Y = d.Z = 1
        d.C = 64
        for n, v in fields.items():
            setattr(d, n, v)
        return ctypes.byref(d)

    assert L.lss_lift_splat_forward_desc(None, None) == -1
    assert L.lss_lift_splat_forward_desc(desc(depth=None), None) == -1
    assert L.lss_lift_splat_forward_desc(desc(C=48), None) == -2
    assert L.lss_lift_splat_forward_desc(desc(layout=7), None) == -3
    # host calibration is an f32-depthnet form
    assert L.lss_lift_splat_forward_desc(desc(x=one, w=one, bias=one, Cin=64, calib_host=one, math=_native.DT_BF16),
                                         None) == -3


def test_exact_index_kernel_has_no_contracted_fma(tmp_path):
    """geom_bucket.hip must be built with -ffp-contract=off - and the ISA it then compiles to
    must really hold no fused multiply-add in the two geometry -> voxel-id kernels (a contracted a*b+c rounds
    once where torch-CPU rounds twice, and flips voxel ids)."""
    import subprocess
    from lss2_multimodal_nu_amd import build_native
    flags = build_native.SOURCES["geom_bucket.hip"]
    assert "-ffp-contract=off" in flags
    asm = tmp_path / "geom_bucket.s"
    subprocess.check_call([build_native._hipcc(), "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(build_native.CSRC, "geom_bucket.hip")] + build_native.COMMON + flags,
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    # IEEE fp32 division (the reference divides by dx, src/model_BEV_TXT.py:92) expands to v_div_scale / v_rcp /
    # FOUR v_fma + ONE v_fmac / v_div_fmas / v_div_fixup: those 5 fused ops per division ARE the correctly rounded
    # quotient.  Any fused op beyond them would be a contracted a*b+c of the geometry arithmetic.
    fused = re.compile(r"\bv_(pk_)?(fma|fmac|mac|mad)_(f32|legacy_f32)")
    seen = 0
    for name in ("points_to_voxels_kernel", "geom_to_voxels_kernel"):
        m = re.search(r"^_ZN[^\n]*%s[^\n]*\n(.*?)s_endpgm" % name, text, flags=re.S | re.M)
        assert m, name
        body = m.group(1)
        ndiv = len(re.findall(r"\bv_div_fmas_f32", body))
        assert ndiv == 3, (name, ndiv)                                   # x, y, z quotients
        assert "v_mul_f32" in body and "v_add_f32" in body, name         # the un-fused arithmetic is there
        assert len(fused.findall(body)) == 5 * ndiv, (name, len(fused.findall(body)))
        seen += 1
    assert seen == 2


def test_no_oracle_import_in_product():
    pkg = os.path.join(ROOT, "lss2_multimodal_nu_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f
