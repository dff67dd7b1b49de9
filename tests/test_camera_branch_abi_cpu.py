"""K13 without a GPU: the header, `_native.SIGNATURES` and the library agree on the three entries and the two structs;
`lss_tapconv_ok`'s truth table; every refusal code of the two launchers on addresses that are never dereferenced (all
checks run before any HIP call); the `ValueError`s of the ops wrappers; the routing of `scene_tokens` / `forward` on CPU
tensors; and the resource usage of the gfx950 code (no scratch)."""
import ctypes
import os
import re
import subprocess
import warnings

import pytest
import torch

from lss2_multimodal_nu_amd import _native as N
from lss2_multimodal_nu_amd import build_native, ops
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_LAYOUT, E_ALIGN = -1, -2, -3, -4
ENTRIES = ("lss_tapconv_ok", "lss_tapconv_fwd", "lss_camera_pool_bias_fwd")


@pytest.fixture(scope="module")
def L():
    build_native.build(verbose=False)
    return N.lib()


def _header():
    return open(os.path.join(ROOT, "include", "lss_hip.h")).read()


def test_header_signatures_and_library_agree(L):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name + " is not declared in include/lss_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):   # pointers are c_void_p, ints are c_int
            assert (a is ctypes.c_void_p) == ("*" in p), (name, p)
        assert hasattr(L, name)
    assert "csrc/camera_branch.hip" in _header() and "camera_branch.hip" in build_native.SOURCES
    assert re.search(r"K13.*?replaces: src/model_vovnet_transformer\.py:176-214, 612-620.*?src/modules\.py:147-207",
                     _header(), flags=re.S)


def test_structs_match_the_header():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for cname, cls in (("lss_tapconv_branch", N.TapconvBranch), ("lss_tapconv_desc", N.TapconvDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % cname, code, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[\d+\]", "", n).strip(" *") for n in decl.split(",")]
        names = [n.split()[-1].strip("*") for n in names]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert ctypes.sizeof(N.TapconvBranch) == 3 * 8 + 4 * 4
    assert ctypes.sizeof(N.TapconvDesc) == 4 * 8 + 4 * ctypes.sizeof(N.TapconvBranch) + 8 * 4


def test_ok_truth_table(L):
    ok = L.lss_tapconv_ok
    for args in ((48, 8, 22, 768, 256), (6, 8, 22, 256, 256), (2, 16, 44, 128, 256), (3, 3, 5, 64, 256),
                 (2, 1, 1, 64, 64), (1, 5, 7, 128, 64), (65535, 1, 1, 4096, 1024), (1, 1024, 64, 64, 64)):
        assert ok(*args) == 1, args
        assert ops.tapconv_ok(*args)
    for args in ((0, 8, 22, 768, 256), (65536, 8, 22, 768, 256), (1, 0, 22, 768, 256), (1, 8, 0, 768, 256),
                 (1, 1025, 1, 64, 64), (1, 1, 1025, 64, 64), (1, 1024, 65, 64, 64), (1, 8, 22, 0, 256),
                 (1, 8, 22, 32, 256), (1, 8, 22, 96, 256), (1, 8, 22, 4160, 256), (1, 8, 22, 768, 0),
                 (1, 8, 22, 768, 32), (1, 8, 22, 768, 100), (1, 8, 22, 768, 1088), (-1, 8, 22, 768, 256)):
        assert ok(*args) == E_SHAPE, args
        assert not ops.tapconv_ok(*args)


def _desc(**kw):
    """A launch every check accepts, on addresses nothing dereferences; `kw` overrides fields, b0_* those of branch 0."""
    d = N.TapconvDesc()
    d.x, d.y = 1024, 2048
    d.BN, d.H, d.W, d.Cin, d.Cout, d.nbranch, d.y_stride, d.relu = 2, 3, 5, 64, 64, 2, 128, 1
    for b in range(2):
        br = d.branch[b]
        br.w, br.scale, br.shift, br.ksize, br.dilation, br.ch_off = 4096, 8192, 16384, 3, 1 + b, 64 * b
    for k, v in kw.items():
        if k.startswith("b0_") or k.startswith("b1_"):
            setattr(d.branch[int(k[1])], k[3:], v)
        else:
            setattr(d, k, v)
    return ctypes.byref(d)


REFUSALS = [
    ("desc_null", None, E_NULL),
    ("x_null", dict(x=None), E_NULL),
    ("no_output", dict(y=None), E_NULL),
    ("w_null", dict(b1_w=None), E_NULL),
    ("nbranch_0", dict(nbranch=0), E_SHAPE),
    ("nbranch_5", dict(nbranch=5), E_SHAPE),
    ("cin_96", dict(Cin=96), E_SHAPE),
    ("cout_48", dict(Cout=48), E_SHAPE),
    ("bn_0", dict(BN=0), E_SHAPE),
    ("relu_2", dict(relu=2), E_LAYOUT),
    ("ksize_2", dict(b0_ksize=2), E_LAYOUT),
    ("ksize_5", dict(b1_ksize=5), E_LAYOUT),
    ("dilation_0", dict(b0_dilation=0), E_SHAPE),
    ("dilation_2000", dict(b0_dilation=2000), E_SHAPE),
    ("means_two_branches", dict(means=64), E_SHAPE),
    ("bias_two_branches", dict(img_bias=64), E_SHAPE),
    ("stride_below_cout", dict(y_stride=32), E_SHAPE),
    ("stride_odd", dict(y_stride=130), E_SHAPE),
    ("ch_off_negative", dict(b0_ch_off=-4), E_SHAPE),
    ("ch_off_unaligned", dict(b0_ch_off=2), E_SHAPE),
    ("ch_off_past_end", dict(b1_ch_off=68), E_SHAPE),
    ("x_unaligned", dict(x=1032), E_ALIGN),
    ("w_unaligned", dict(b0_w=4104), E_ALIGN),
    ("scale_unaligned", dict(b0_scale=8196), E_ALIGN),
    ("shift_unaligned", dict(b1_shift=16392), E_ALIGN),
    ("y_unaligned", dict(y=2052), E_ALIGN),
    ("bias_unaligned", dict(nbranch=1, img_bias=72), E_ALIGN),
    ("means_unaligned", dict(nbranch=1, means=66), E_ALIGN),
]


@pytest.mark.parametrize("what,fields,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_tapconv_refusals(L, what, fields, code):
    assert L.lss_tapconv_fwd(None if fields is None else _desc(**fields), None) == code
    assert L.lss_error_string(code)


def test_pool_bias_refusals(L):
    p = ctypes.c_void_p
    good = [p(64), p(128), p(192), p(256), p(320), 2, 256, 256, 256, p(384), p(448), None]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.lss_camera_pool_bias_fwd(*a)

    for i in (0, 1, 4, 10):                       # mean, wg, wj, bias are required; scale, shift, g are not
        assert call(**{"a%d" % i: None}) == E_NULL
    for i, v in ((5, 0), (5, 65536), (6, 0), (6, 1025), (7, 0), (7, 1025), (8, 0), (8, 4097)):
        assert call(**{"a%d" % i: v}) == E_SHAPE, (i, v)
    for i in (0, 1, 2, 3, 4, 9, 10):
        assert call(**{"a%d" % i: p(good[i].value + 2)}) == E_ALIGN, i


def test_wrapper_value_errors():
    x = torch.zeros(1, 3, 5, 64, dtype=torch.bfloat16)
    w = torch.zeros(9, 64, 64, dtype=torch.bfloat16)
    sc = torch.ones(64)
    br = (w, 3, 1, sc, sc, 0)
    with pytest.raises(ValueError):               # CPU tensors never reach the library
        ops.tapconv(x, [br], y=torch.zeros(1, 3, 5, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.tapconv(x.float(), [br], means=True)
    with pytest.raises(ValueError):
        ops.tapconv(x[..., ::2], [br], means=True)
    with pytest.raises(ValueError):
        ops.camera_pool_bias(torch.zeros(2, 256), torch.zeros(256, 256), None, None, torch.zeros(256, 256))
    with pytest.raises(ValueError):
        ops.camera_pool_bias(torch.zeros(256), torch.zeros(256, 256), None, None, torch.zeros(256, 256))


def test_scene_tokens_on_cpu_takes_the_composition(monkeypatch):
    """CPU maps: `scene_tokens` and `forward` take the two library lines, count them, and K13 is never asked."""

    class Trunk(mv.TrunkC3C4):
        c3_channels, c4_channels = 64, 128

    grid = dict(xbound=[-50.0, 50.0, 2.0], ybound=[-50.0, 50.0, 2.0], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
    conf = dict(final_dim=(64, 96), Ncams=2, cams=["A", "B"])
    torch.manual_seed(0)
    m = mv.VoVNetBEVTransformer(1, grid, conf, outC=4, backbone=Trunk(), precision="bf16").eval()
    monkeypatch.setattr(ops, "tapconv", lambda *a, **k: pytest.fail("K13 used on CPU tensors"))
    monkeypatch.setattr(mv.VoVNetBEVTransformer, "get_voxels", lambda self, *a, **k: torch.zeros(1, 128, 50, 50))
    c3, c4 = torch.randn(2, 64, 4, 6), torch.randn(2, 128, 2, 3)
    before = dict(mv.CAMERA_BRANCH_CALLS)
    with torch.no_grad():
        tok = m.scene_tokens(c3)
        want = m.sceneunder(m.feature_pyramid(c3)).mean(dim=(2, 3))
    assert tok.shape == (2, 256) and tok.dtype == torch.float32 and torch.equal(tok, want)
    assert mv.CAMERA_BRANCH_CALLS == {"native": before["native"], "composition": before["composition"] + 1}
    calib = [torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3, 3),
             torch.zeros(1, 2, 3)]
    with warnings.catch_warnings():               # eval mode with autograd on: the differentiable route, on the CPU
        warnings.simplefilter("ignore")           # (it warns once per module class that this is not the fused path)
        seg, action, description = m({"c3": c3, "c4": c4}, *calib)
    assert action.shape == (1, 4) and description.shape == (1, 8)
    assert mv.CAMERA_BRANCH_CALLS == {"native": before["native"], "composition": before["composition"] + 2}


def test_structure_check_refuses_foreign_modules():
    fp, su = mv.AdaptiveFeaturePyramid(64, 256), mv.SceneUnder(in_channels=256)
    assert mv._CameraBranchPlan.convs_of(fp, su) is not None
    assert mv._CameraBranchPlan.convs_of(mv.AdaptiveFeaturePyramid(64, 128), su) is None          # 128 mid channels
    assert mv._CameraBranchPlan.convs_of(fp, mv.SceneUnder(in_channels=512)) is None              # BEV_TXT's SceneUnder
    assert mv._CameraBranchPlan.convs_of(fp, torch.nn.Sequential(torch.nn.Identity())) is None
    from lss2_multimodal_nu_amd.heads import ASPP
    assert mv._CameraBranchPlan.convs_of(fp, torch.nn.Sequential(ASPP(256, [6, 12, 18]))) is not None   # any three rates
    assert mv._CameraBranchPlan.convs_of(fp, torch.nn.Sequential(ASPP(256, [6, 12]))) is None


def test_kernels_use_no_scratch(tmp_path):
    """Resource usage of the gfx950 code of camera_branch.hip: no private segment, no spills, and the ring of the conv
    kernel leaves room for four workgroups per CU."""
    asm = tmp_path / "camera_branch.s"
    subprocess.check_call([build_native._hipcc(), "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(build_native.CSRC, "camera_branch.hip")] + build_native.COMMON
                          + build_native.SOURCES["camera_branch.hip"], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    kernels = [k for k in re.findall(r"\.name:\s+(\S*(?:tapconv|pool_bias)_kernel\S*)\n", text) if not k.endswith(".kd")]
    assert len(kernels) == 2, kernels
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert len(private) == 2 and private == [0, 0]
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) <= 40 * 1024 for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text))
    assert "v_mfma_f32_16x16x32_bf16" in text
