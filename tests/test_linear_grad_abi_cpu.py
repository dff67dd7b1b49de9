"""CPU-side checks of K11 (lss_linear_wgrad, lss_layernorm_bwd and their _ok / _workspace_bytes queries): header <->
_native.SIGNATURES <-> the built library, the argument checks (they run before any HIP call), the documented limits and
split rules, the Python wrappers' own checks, the encoder layer's route on CPU tensors, and the kernels' resources."""
import ctypes
import os
import re

import pytest
import torch

import transformer_grad_ref as G

E_NULL, E_SHAPE, E_LAYOUT, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4, -5
NAMES = ("lss_linear_wgrad", "lss_linear_wgrad_ok", "lss_linear_wgrad_workspace_bytes",
         "lss_layernorm_bwd", "lss_layernorm_bwd_ok", "lss_layernorm_bwd_workspace_bytes")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from lss2_multimodal_nu_amd import _native, build_native
    build_native.build(verbose=False)
    return _native.lib()


def _p(addr):
    return ctypes.c_void_p(addr)


A = _p(1 << 20)  # an aligned (never dereferenced) address
_CTYPE = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "float": ctypes.c_float}


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "lss_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(lss_(?:linear_wgrad|layernorm_bwd)\w*)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            types.append(ctypes.c_void_p if "*" in a else _CTYPE[a.rsplit(" ", 1)[0].replace("const ", "")])
        out[name] = (_CTYPE[ret], types)
    return out


def test_header_signatures_library_agree(L):
    from lss2_multimodal_nu_amd import _native
    protos = _header_prototypes()
    assert sorted(protos) == sorted(NAMES)
    for name in NAMES:
        assert name in _native.SIGNATURES, name
        res, args = _native.SIGNATURES[name]
        assert (res, list(args)) == (protos[name][0], protos[name][1]), name
        fn = getattr(L, name)  # AttributeError = the symbol is not in the built library
        assert fn.restype is res and list(fn.argtypes) == list(args)
    hdr = open(os.path.join(ROOT, "include", "lss_hip.h")).read()
    k11 = hdr[hdr.index("K11"):hdr.index("int lss_linear_wgrad_ok")]
    assert "replaces:" in k11 and "src/transformer_modules.py:77-84" in k11 and ":170-215" in k11
    assert "train_vovnet_transformer.py:210" in k11


def test_linear_wgrad_ok_and_workspace_follow_the_documented_rule(L):
    good = [(1, 64, 64), (33, 64, 64), (300, 64, 64), (4551, 192, 256), (4551, 256, 256), (1250, 1024, 256),
            (1250, 256, 1024), (40000, 256, 256), (320000, 1024, 256), (1 << 22, 1024, 1024), (129, 64, 1024)]
    for T, N, K in good:
        assert L.lss_linear_wgrad_ok(T, N, K) == 1 and G.wgrad_ok(T, N, K)
        assert L.lss_linear_wgrad_workspace_bytes(T, N, K) == G.wgrad_workspace_bytes(T, N, K), (T, N, K)
    # the split count never exceeds one workgroup pair per CU and never leaves a split without a stage
    for T, N, K in good:
        sp = G.wgrad_split(T, N, K)
        assert 1 <= sp.splits <= max(1, 512 // ((N // 64) * (K // 64))) and (sp.splits - 1) * sp.per < sp.stages
    bad = [(0, 64, 64), (-1, 64, 64), ((1 << 22) + 1, 64, 64), (8, 0, 64), (8, 64, 0), (8, 32, 64), (8, 64, 32),
           (8, 96, 64), (8, 64, 100), (8, 1088, 64), (8, 64, 1088)]
    for T, N, K in bad:
        assert L.lss_linear_wgrad_ok(T, N, K) == 0 and not G.wgrad_ok(T, N, K)
        assert L.lss_linear_wgrad_workspace_bytes(T, N, K) == 0


def test_layernorm_bwd_ok_and_workspace(L):
    for rows in (1, 4, 5, 257, 4551, 320000, (1 << 31) - 1):
        assert L.lss_layernorm_bwd_ok(rows, 256) == 1
        assert L.lss_layernorm_bwd_workspace_bytes(rows) == G.ln_bwd_groups(rows) * 2 * 256 * 4
    for rows, Cc in ((0, 256), (-3, 256), (1 << 31, 256), (8, 128), (8, 512)):
        assert L.lss_layernorm_bwd_ok(rows, Cc) == 0
    assert L.lss_layernorm_bwd_workspace_bytes(0) == 0


def wgrad(L, x=A, dy=A, T=300, N=64, K=64, ws=A, wsb=None, dw=A, db=A):
    if wsb is None:
        wsb = L.lss_linear_wgrad_workspace_bytes(T, N, K)
    return L.lss_linear_wgrad(x, dy, T, N, K, ws, wsb, dw, db, None)


def test_linear_wgrad_argument_checks(L):
    assert wgrad(L, dy=None) == E_NULL
    assert wgrad(L, x=None) == E_NULL          # dw asked for
    assert wgrad(L, ws=None) == E_NULL
    assert wgrad(L, dw=None, db=None) == E_NULL  # nothing asked for
    for kw in (dict(T=0), dict(T=(1 << 22) + 1), dict(N=96), dict(K=32), dict(N=1088), dict(K=0)):
        assert wgrad(L, wsb=1 << 30, **kw) == E_SHAPE, kw
    assert wgrad(L, x=_p((1 << 20) + 8)) == E_ALIGN       # 16-B loads
    assert wgrad(L, dy=_p((1 << 20) + 2)) == E_ALIGN
    assert wgrad(L, ws=_p((1 << 20) + 4)) == E_ALIGN
    assert wgrad(L, dw=_p((1 << 20) + 2)) == E_ALIGN
    assert wgrad(L, db=_p((1 << 20) + 1)) == E_ALIGN
    assert wgrad(L, wsb=L.lss_linear_wgrad_workspace_bytes(300, 64, 64) - 1) == E_WORKSPACE
    assert wgrad(L, wsb=0) == E_WORKSPACE


def lnb(L, x=A, xdt=0, dy=A, gdt=0, gamma=A, rows=5, Cc=256, ws=A, wsb=None, dx=A, odt=0, dg=A, db=A):
    if wsb is None:
        wsb = L.lss_layernorm_bwd_workspace_bytes(rows)
    return L.lss_layernorm_bwd(x, xdt, dy, gdt, gamma, rows, Cc, 1e-5, ws, wsb, dx, odt, dg, db, None)


def test_layernorm_bwd_argument_checks(L):
    for name in ("x", "dy", "gamma", "ws", "dx", "dg", "db"):
        assert lnb(L, **{name: None}) == E_NULL, name
    assert lnb(L, rows=0, wsb=4096) == E_SHAPE
    assert lnb(L, Cc=128) == E_SHAPE
    for name in ("xdt", "gdt", "odt"):
        assert lnb(L, **{name: 2}) == E_LAYOUT and lnb(L, **{name: -1}) == E_LAYOUT
    for name in ("x", "dy", "gamma", "dx", "ws"):
        assert lnb(L, **{name: _p((1 << 20) + 8)}) == E_ALIGN, name
    assert lnb(L, dg=_p((1 << 20) + 2)) == E_ALIGN
    assert lnb(L, wsb=L.lss_layernorm_bwd_workspace_bytes(5) - 1) == E_WORKSPACE


def test_wrappers_reject_before_the_library():
    from lss2_multimodal_nu_amd import ops
    x, dy = torch.zeros(8, 64).bfloat16(), torch.zeros(8, 128).bfloat16()
    for kw in (dict(x=x.float()), dict(dy=dy.float()), dict(x=x[:, :32]), dict(x=x[:4]), dict(x=x[None]),
               dict(want_dw=False, want_db=False), dict(dy=torch.zeros(8, 96).bfloat16()),
               dict(x=torch.zeros(8, 1088).bfloat16()), dict()):          # the last: everything right except the device
        a = dict(x=x, dy=dy)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.linear_wgrad(a.pop("x"), a.pop("dy"), **a)
    r, g, gamma = torch.zeros(3, 256), torch.zeros(3, 256), torch.ones(256)
    for kw in (dict(x=r.double()), dict(dy=g.half()), dict(dy=g[:2]), dict(x=torch.zeros(3, 128), dy=torch.zeros(3, 128)),
               dict(dx_dtype=torch.float16), dict()):
        a = dict(x=r, dy=g, dx_dtype=torch.float32)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.layernorm_bwd(a["x"], a["dy"], gamma, 1e-5, a["dx_dtype"])


def test_encoder_layer_on_cpu_tensors_takes_the_composition(monkeypatch):
    """bf16 autocast on the CPU: no GPU tensor, so the native nodes are not used and the torch composition runs and
    differentiates; the counter says so."""
    from lss2_multimodal_nu_amd import transformer_modules as tm
    monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", "1")
    monkeypatch.setattr(tm._LinearFn, "forward", lambda *a, **k: pytest.fail("native node used on CPU tensors"))
    torch.manual_seed(0)
    layer = tm.TransformerEncoderLayer(256, 8, 128, 0.0).train()
    src = torch.randn(1, 16, 256, requires_grad=True)
    pos = torch.randn(1, 256, 4, 4)
    ref = tm.LightweightBEVTransformer.reference_points(4, 4, "cpu")
    before = dict(tm.TRANSFORMER_CALLS)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out = layer(src, pos, ref)
    out.float().sum().backward()
    assert tm.TRANSFORMER_CALLS["composition"] == before["composition"] + 1
    assert tm.TRANSFORMER_CALLS["native"] == before["native"]
    assert src.grad is not None and layer.linear1.weight.grad is not None


def test_kernels_use_no_scratch(tmp_path):
    """Resource usage of the gfx950 code: no kernel of linear_grad.hip has a private (scratch) segment or spills vector
    registers; the weight-gradient kernel's 64 KiB of LDS leave room for two workgroups per CU."""
    import subprocess
    from lss2_multimodal_nu_amd import build_native
    asm = tmp_path / "linear_grad.s"
    subprocess.check_call([build_native._hipcc(), "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(build_native.CSRC, "linear_grad.hip")] + build_native.COMMON
                          + build_native.SOURCES["linear_grad.hip"], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    kernels = [k for k in re.findall(r"\.name:\s+(\S+_kernel\S*)\n", text) if not k.endswith(".kd")]
    assert len(kernels) == 2, kernels   # wgrad + its reduce (the LayerNorm backward is in transformer_pointwise.hip)
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text))
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) <= 64 * 1024 for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text))
    assert "ds_read_b64_tr_b16" in text and "v_mfma_f32_16x16x32_bf16" in text
