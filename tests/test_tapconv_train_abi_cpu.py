"""K16 and the camera branch's training route without a GPU: the header, `_native.SIGNATURES` and the library agree on
the four entries; `lss_tapconv_wgrad_ok`'s truth table and its consistency with the workspace size; every refusal code
of the two launchers on addresses that are never dereferenced (all checks run before any HIP call, so nothing can be
written); the `ValueError`s of the ops wrappers; the Python guards; the routing of a training `scene_tokens` call to the
composition, asserted on CAMERA_BRANCH_TRAIN_CALLS; and the resource usage of the gfx950 code (no scratch)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from lss2_multimodal_nu_amd import _native as N
from lss2_multimodal_nu_amd import build_native, modules, ops
from lss2_multimodal_nu_amd import model_vovnet_transformer as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_LAYOUT, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4, -5
ENTRIES = {"lss_tapconv_wgrad_ok": "int", "lss_tapconv_wgrad_workspace_bytes": "size_t", "lss_tapconv_wgrad": "int",
           "lss_tapconv_bias_grad": "int"}


@pytest.fixture(scope="module")
def L():
    build_native.build(verbose=False)
    return N.lib()


def _header():
    return open(os.path.join(ROOT, "include", "lss_hip.h")).read()


def test_header_signatures_and_library_agree(L):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, rtype in ENTRIES.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (rtype, name), code)
        assert m, name + " is not declared in include/lss_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = N.SIGNATURES[name]
        assert res is (ctypes.c_int if rtype == "int" else ctypes.c_size_t) and len(args) == len(params), name
        for p, a in zip(params, args):
            assert (a is ctypes.c_void_p) == ("*" in p), (name, p)
            assert (a is ctypes.c_size_t) == p.startswith("size_t"), (name, p)
        assert hasattr(L, name)
    assert "csrc/tapconv_wgrad.hip" in _header() and "tapconv_wgrad.hip" in build_native.SOURCES
    assert re.search(r"K16.*?H W <= 224", _header(), flags=re.S)      # the bound is stated in the header


def test_ok_truth_table_and_workspace(L):
    ok, wsb = L.lss_tapconv_wgrad_ok, L.lss_tapconv_wgrad_workspace_bytes
    for args in ((48, 8, 22, 768, 256), (6, 8, 22, 1024, 256), (2, 5, 9, 64, 64), (1, 1, 1, 64, 64), (3, 14, 16, 128, 64),
                 (65535, 1, 224, 4096, 1024), (1, 224, 1, 64, 64)):
        assert ok(*args) == 1 and ops.tapconv_wgrad_ok(*args), args
        assert L.lss_tapconv_ok(*args) == 1                       # nothing K16 takes is refused by the forward conv
        for k, d, ntap in ((1, 1, 1), (3, 1, None), (3, 1024, 1)):
            n = wsb(*args, k, d)
            live = len(ops.live_taps(args[1], args[2], k, d))
            assert ntap is None or live == ntap
            assert n > 0 and n % (4 * live * args[3] * args[4]) == 0
            assert 1 <= n // (4 * live * args[3] * args[4]) <= args[0]      # 1 .. BN splits
        assert wsb(*args, 2, 1) == 0 and wsb(*args, 3, 0) == 0 and wsb(*args, 3, 1025) == 0
    for args in ((0, 8, 22, 768, 256), (65536, 8, 22, 768, 256), (1, 0, 22, 64, 64), (1, 8, 0, 64, 64), (1, 15, 15, 64, 64),
                 (1, 1, 225, 64, 64), (1, 225, 1, 64, 64), (1, 16, 44, 64, 64), (1, 65536, 65536, 64, 64),
                 (1, 8, 22, 96, 64), (1, 8, 22, 32, 64), (1, 8, 22, 4160, 64), (1, 8, 22, 64, 48), (1, 8, 22, 64, 1088),
                 (-1, 8, 22, 64, 64)):
        assert ok(*args) == E_SHAPE and not ops.tapconv_wgrad_ok(*args), args
        assert wsb(*args, 3, 1) == 0
    assert wsb(48, 8, 22, 768, 256, 3, 2) == 10 * 9 * 768 * 256 * 4     # 48 tiles: 10 image ranges of 5, nine live taps
    assert wsb(48, 8, 22, 256, 256, 3, 12) == 24 * 3 * 256 * 256 * 4    # 16 tiles: 24 ranges of 2, a 1 x 3


p = ctypes.c_void_p
GOOD_W = [p(1024), p(2048), 2, 5, 9, 64, 64, 3, 2, p(4096), 1 << 30, p(8192), None]
WGRAD_REFUSALS = [
    ("x_null", {0: None}, E_NULL), ("dy_null", {1: None}, E_NULL), ("ws_null", {9: None}, E_NULL),
    ("dw_null", {11: None}, E_NULL),
    ("bn_0", {2: 0}, E_SHAPE), ("h_0", {3: 0}, E_SHAPE), ("hw_225", {3: 15, 4: 15}, E_SHAPE), ("cin_96", {5: 96}, E_SHAPE),
    ("cout_48", {6: 48}, E_SHAPE), ("cout_1088", {6: 1088}, E_SHAPE), ("dilation_0", {8: 0}, E_SHAPE),
    ("dilation_2000", {8: 2000}, E_SHAPE),
    ("ksize_2", {7: 2}, E_LAYOUT), ("ksize_5", {7: 5}, E_LAYOUT), ("ksize_0", {7: 0}, E_LAYOUT),
    ("x_unaligned", {0: p(1032)}, E_ALIGN), ("dy_unaligned", {1: p(2056)}, E_ALIGN), ("ws_unaligned", {9: p(4104)}, E_ALIGN),
    ("dw_unaligned", {11: p(8194)}, E_ALIGN),
    ("ws_small", {10: 2 * 9 * 64 * 64 * 4 - 1}, E_WORKSPACE), ("ws_zero", {10: 0}, E_WORKSPACE),
]


@pytest.mark.parametrize("what,change,code", WGRAD_REFUSALS, ids=[r[0] for r in WGRAD_REFUSALS])
def test_wgrad_refusals(L, what, change, code):
    a = list(GOOD_W)
    for i, v in change.items():
        a[i] = v
    assert L.lss_tapconv_wgrad(*a) == code
    assert L.lss_error_string(code)


def test_wgrad_refusal_leaves_real_buffers_untouched(L):
    """The same refusals on real host buffers: a refused call writes neither the workspace nor dw."""
    x = torch.zeros(2 * 5 * 9 * 64, dtype=torch.bfloat16)
    ws = torch.full((2 * 9 * 64 * 64,), 7.0)
    dw = torch.full((64 * 64 * 9,), 7.0)
    for change in ({7: 4}, {8: 0}, {5: 96}, {10: 16}):
        a = [p(x.data_ptr()), p(x.data_ptr()), 2, 5, 9, 64, 64, 3, 2, p(ws.data_ptr()), ws.numel() * 4, p(dw.data_ptr()), None]
        for i, v in change.items():
            a[i] = v
        assert L.lss_tapconv_wgrad(*a) < 0
        assert bool((ws == 7.0).all()) and bool((dw == 7.0).all())


def test_bias_grad_refusals(L):
    good = [p(1024), 2, 5, 9, 64, p(2048), None]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.lss_tapconv_bias_grad(*a)

    assert call(a0=None) == E_NULL and call(a5=None) == E_NULL
    for i, v in ((1, 0), (1, 65536), (2, 0), (3, 0), (2, 1025), (3, 1025), (4, 0), (4, 32), (4, 96), (4, 1088)):
        assert call(**{"a%d" % i: v}) == E_SHAPE, (i, v)
    assert call(a2=1024, a3=65) == E_SHAPE
    assert call(a0=p(1032)) == E_ALIGN and call(a5=p(2050)) == E_ALIGN
    out = torch.full((2 * 64,), 7.0)
    assert call(a5=p(out.data_ptr()), a4=96) == E_SHAPE and bool((out == 7.0).all())


def test_wrapper_value_errors():
    x = torch.zeros(1, 3, 5, 64, dtype=torch.bfloat16)
    for args in ((x, x, 3, 1), (x.float(), x, 3, 1), (x[..., ::2], x, 3, 1)):     # CPU tensors never reach the library
        with pytest.raises(ValueError):
            ops.tapconv_wgrad(*args)
    with pytest.raises(ValueError):
        ops.tapconv_bias_grad(x)


def _unit(k=3, d=2, cin=64, cout=64, bias=True):
    conv = torch.nn.Conv2d(cin, cout, k, padding=d if k == 3 else 0, dilation=d, bias=bias)
    return conv, torch.nn.BatchNorm2d(cout)


def test_unit_guard(monkeypatch):
    """`_tapconv_unit_ok` on stand-in GPU maps (the guard reads is_cuda, dim() and shape only): bf16 autocast is what
    `_native_training` reports, patched in here; everything else is the guard's own."""
    x = mv._MapLike(2, 64, 5, 9)
    conv, bn = _unit()
    assert not modules._tapconv_unit_ok(conv, bn, x)                  # no bf16 autocast on this machine
    monkeypatch.setattr(modules, "_native_training", lambda: True)
    assert modules._tapconv_unit_ok(conv, bn, x)
    assert modules._tapconv_unit_ok(*_unit(k=1, d=1), x)
    assert modules._tapconv_unit_ok(*_unit(d=12, bias=False), x)
    assert not modules._tapconv_unit_ok(conv, bn, torch.zeros(2, 64, 5, 9))          # a CPU tensor
    assert not modules._tapconv_unit_ok(conv, bn, mv._MapLike(2, 64, 15, 15))        # H W > 224
    assert not modules._tapconv_unit_ok(conv, bn, mv._MapLike(2, 128, 5, 9))         # not the conv's input width
    assert not modules._tapconv_unit_ok(*_unit(cin=96), mv._MapLike(2, 96, 5, 9))
    assert not modules._tapconv_unit_ok(*_unit(cout=32), x)
    bn.eval()
    assert not modules._tapconv_unit_ok(conv, bn, x)                  # an eval-mode BatchNorm does not take batch statistics
    bn.train()
    modules.enable_sync_bn(bn)
    assert not modules._tapconv_unit_ok(conv, bn, x)                  # statistics over ranks
    modules.enable_sync_bn(bn, False)
    assert modules._tapconv_unit_ok(conv, bn, x)
    for bad in (torch.nn.Conv2d(64, 64, 3, padding=1, dilation=2), torch.nn.Conv2d(64, 64, 3, padding=2, dilation=2, stride=2),
                torch.nn.Conv2d(64, 64, 3, padding=(2, 1), dilation=(2, 1)), torch.nn.Conv2d(64, 64, 3, padding=2, dilation=2, groups=2),
                torch.nn.Conv2d(64, 64, 5, padding=2), torch.nn.Conv2d(64, 64, 1, padding=1),
                torch.nn.Conv2d(64, 64, 3, padding=2, dilation=2, padding_mode="reflect"),
                torch.nn.Conv2d(64, 64, 3, padding=2, dilation=2).half()):
        assert not modules._tapconv_unit_ok(bad, bn, x), bad
    wide = torch.nn.Conv2d(320, 64, 1, bias=False)                     # the projection: 256 of 320 input channels
    assert modules._tapconv_unit_ok(wide, bn, mv._MapLike(2, 256, 5, 9), cin=256)
    assert not modules._tapconv_unit_ok(wide, bn, mv._MapLike(2, 256, 5, 9))
    monkeypatch.undo()
    assert not modules._tapconv_unit_ok(conv, bn, x)


class _Trunk(mv.TrunkC3C4):
    c3_channels, c4_channels = 64, 128


def _model():
    grid = dict(xbound=[-50.0, 50.0, 2.0], ybound=[-50.0, 50.0, 2.0], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
    torch.manual_seed(0)
    return mv.VoVNetBEVTransformer(1, grid, dict(final_dim=(64, 96), Ncams=2, cams=["A", "B"]), outC=4, backbone=_Trunk(),
                                   precision="bf16").train()


def test_counter_has_exactly_two_keys_and_the_old_one_is_unchanged():
    assert set(mv.CAMERA_BRANCH_TRAIN_CALLS) == {"native", "composition"}
    assert set(mv.CAMERA_BRANCH_CALLS) == {"native", "composition"}


def test_training_calls_without_a_gpu_take_the_composition(monkeypatch):
    """CPU maps, with and without autocast: a training call is the two library lines, counted on the new counter (and,
    as before, on CAMERA_BRANCH_CALLS); the native units are never asked."""
    m = _model()
    monkeypatch.setattr(modules, "_train_tapconv_bn_act", lambda *a, **k: pytest.fail("native unit used on CPU tensors"))
    c3 = torch.randn(2, 64, 4, 6, requires_grad=True)
    for ctx in (torch.autocast("cpu", torch.bfloat16), torch.autocast("cpu", enabled=False)):
        before, old = dict(mv.CAMERA_BRANCH_TRAIN_CALLS), dict(mv.CAMERA_BRANCH_CALLS)
        with ctx:
            tok = m.scene_tokens(c3)
        assert tok.shape == (2, 256) and tok.requires_grad
        assert mv.CAMERA_BRANCH_TRAIN_CALLS == {"native": before["native"], "composition": before["composition"] + 1}
        assert mv.CAMERA_BRANCH_CALLS == {"native": old["native"], "composition": old["composition"] + 1}
    m.eval()
    before = dict(mv.CAMERA_BRANCH_TRAIN_CALLS)
    with torch.no_grad():
        m.scene_tokens(c3.detach())                   # an inference call is not a training call
    assert mv.CAMERA_BRANCH_TRAIN_CALLS == before


def test_route_guard_on_stand_in_gpu_maps(monkeypatch):
    """`_camera_branch_train_native_ok` with the device questions answered as on the GPU (a c3 that says it is a GPU
    tensor, bf16 autocast reported on, device equality patched away): the reference structure in training mode
    passes; fp16 autocast, an eval-mode BatchNorm, a hooked child, `_lss_sync`, a foreign width, no autograd and the
    switch each refuse.  On the real route every refusal is a composition call: asserted through `scene_tokens`."""
    m = _model()
    autocast = {"on": True}
    monkeypatch.setattr(modules, "_native_training", lambda: autocast["on"])

    class FakeGpu(torch.Tensor):
        is_cuda = True

    c3 = torch.randn(2, 64, 4, 6).as_subclass(FakeGpu)
    ok = lambda: m._camera_branch_train_native_ok(c3)  # noqa: E731
    assert ok()
    autocast["on"] = False                               # fp16 autocast or none: `_native_training` is false
    assert not ok()
    autocast["on"] = True
    bn = m.sceneunder[0].convs[2][1]
    bn.eval()
    assert not ok()
    bn.train()
    h = m.feature_pyramid.scale2[0].register_forward_hook(lambda *a: None)
    assert not ok()
    h.remove()
    h = m.sceneunder[0].project[3].register_forward_pre_hook(lambda *a: None)
    assert not ok()
    h.remove()
    assert ok()
    modules.enable_sync_bn(m.feature_pyramid.scale2[1])
    assert not ok()
    modules.enable_sync_bn(m.feature_pyramid.scale2[1], False)
    assert ok()
    with torch.no_grad():
        assert not ok()
    monkeypatch.setenv("LSS_CAMERA_BRANCH_TRAIN_NATIVE", "0")
    assert not ok()
    monkeypatch.delenv("LSS_CAMERA_BRANCH_TRAIN_NATIVE")
    assert not m._camera_branch_train_native_ok(torch.randn(2, 64, 16, 16).as_subclass(FakeGpu))    # H W > 224
    m.sceneunder[0].convs[1][0].weight.data = m.sceneunder[0].convs[1][0].weight.data.half()
    assert not ok()
    # every refusal above is a composition call on the counters
    for setup in ("eval_bn", "hook", "sync"):
        m = _model()
        hook = None
        if setup == "eval_bn":
            m.sceneunder[0].convs[2][1].eval()
        elif setup == "hook":
            hook = m.feature_pyramid.fusion.register_forward_hook(lambda *a: None)
        else:
            modules.enable_sync_bn(m.sceneunder[0].project[1])
        before = dict(mv.CAMERA_BRANCH_TRAIN_CALLS)
        m.scene_tokens(torch.randn(2, 64, 4, 6))
        assert mv.CAMERA_BRANCH_TRAIN_CALLS == {"native": before["native"], "composition": before["composition"] + 1}, setup
        if hook is not None:
            hook.remove()


def test_kernels_use_no_scratch(tmp_path):
    """Resource usage of the gfx950 code of tapconv_wgrad.hip: no private segment, no spills, LDS within the static
    64 KiB, transposed LDS reads and bf16 MFMAs in the code."""
    asm = tmp_path / "tapconv_wgrad.s"
    subprocess.check_call([build_native._hipcc(), "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(build_native.CSRC, "tapconv_wgrad.hip")] + build_native.COMMON
                          + build_native.SOURCES["tapconv_wgrad.hip"], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    kernels = [k for k in re.findall(r"\.name:\s+(\S*tapconv_(?:wgrad|wgrad_reduce|bias_grad)_kernel\S*)\n", text)
               if not k.endswith(".kd")]
    assert len(kernels) == 3, kernels
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert private == [0, 0, 0]
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) <= 64 * 1024 for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text))
    assert "v_mfma_f32_16x16x32_bf16" in text and "ds_read_b64_tr_b16" in text
    assert "atomic" not in text.split(".amdgpu_metadata")[0]
