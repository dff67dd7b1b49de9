"""CPU-side checks of K12 (lss_gelu_dropout_fwd / _bwd, lss_add_dropout_ln_fwd / _bwd and their queries): header <->
_native.SIGNATURES <-> the built library, the argument checks (they run before any HIP call, on never-dereferenced
addresses), the documented limits and workspace rule, the Python wrappers' own checks, the encoder layer's route on CPU
tensors, and the kernels' resources."""
import ctypes
import os
import re

import pytest
import torch

import transformer_grad_ref as G

E_NULL, E_SHAPE, E_LAYOUT, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4, -5
NAMES = ("lss_gelu_dropout_ok", "lss_gelu_dropout_fwd", "lss_gelu_dropout_bwd", "lss_add_dropout_ln_ok",
         "lss_add_dropout_ln_bwd_workspace_bytes", "lss_add_dropout_ln_fwd", "lss_add_dropout_ln_bwd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from lss2_multimodal_nu_amd import _native, build_native
    build_native.build(verbose=False)
    return _native.lib()


def _p(addr):
    return ctypes.c_void_p(addr)


A, B = _p(1 << 20), _p(2 << 20)  # aligned (never dereferenced) addresses
_CTYPE = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "float": ctypes.c_float}


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "lss_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(lss_(?:gelu_dropout|add_dropout_ln)\w*)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            types.append(ctypes.c_void_p if "*" in a else _CTYPE[a.rsplit(" ", 1)[0].replace("const ", "")])
        out[name] = (_CTYPE[ret], types)
    return out


def test_header_signatures_library_agree(L):
    from lss2_multimodal_nu_amd import _native, build_native
    protos = _header_prototypes()
    assert sorted(protos) == sorted(NAMES)
    for name in NAMES:
        assert name in _native.SIGNATURES, name
        res, args = _native.SIGNATURES[name]
        assert (res, list(args)) == (protos[name][0], protos[name][1]), name
        fn = getattr(L, name)  # AttributeError = the symbol is not in the built library
        assert fn.restype is res and list(fn.argtypes) == list(args)
    hdr = open(os.path.join(ROOT, "include", "lss_hip.h")).read()
    k12 = hdr[hdr.index("K12"):hdr.index("int lss_gelu_dropout_ok")]
    assert "replaces:" in k12 and "src/transformer_modules.py:207-208, 211-213" in k12
    assert "transformer_pointwise.hip" in build_native.SOURCES


def test_ok_queries_and_workspace(L):
    for n in (8, 64, 257 * 1024, 320000 * 1024, 1 << 32):
        assert L.lss_gelu_dropout_ok(n) == 1
    for n in (0, -8, 4, 12, (1 << 32) + 8):
        assert L.lss_gelu_dropout_ok(n) == 0
    for rows in (1, 4, 5, 257, 4551, 320000, 1 << 22):
        assert L.lss_add_dropout_ln_ok(rows, 256) == 1
        # lss_layernorm_bwd's partials: the same row ranges
        assert L.lss_add_dropout_ln_bwd_workspace_bytes(rows) == G.ln_bwd_groups(rows) * 2 * 256 * 4
        assert L.lss_add_dropout_ln_bwd_workspace_bytes(rows) == L.lss_layernorm_bwd_workspace_bytes(rows)
    for rows, Cc in ((0, 256), (-3, 256), ((1 << 22) + 1, 256), (8, 128), (8, 512)):
        assert L.lss_add_dropout_ln_ok(rows, Cc) == 0
    assert L.lss_add_dropout_ln_bwd_workspace_bytes(0) == 0
    assert L.lss_add_dropout_ln_bwd_workspace_bytes((1 << 22) + 1) == 0


def gd_fwd(L, h=A, n=64, thr=6554, scale=1.1, seed=A, y=B):
    return L.lss_gelu_dropout_fwd(h, n, thr, scale, seed, y, None)


def gd_bwd(L, h=A, dy=_p(3 << 20), n=64, thr=6554, scale=1.1, seed=A, dh=B):
    return L.lss_gelu_dropout_bwd(h, dy, n, thr, scale, seed, dh, None)


def test_gelu_dropout_argument_checks(L):
    for fn, names in ((gd_fwd, ("h", "y")), (gd_bwd, ("h", "dy", "dh"))):
        for name in names:
            assert fn(L, **{name: None}) == E_NULL, name
        for n in (0, 4, 12, -8, (1 << 32) + 8):
            assert fn(L, n=n) == E_SHAPE, n
        for thr in (-1, 65536, 1 << 20):
            assert fn(L, thr=thr) == E_SHAPE, thr          # p so close to 1 that nothing would be kept, or negative
        for name in names:
            assert fn(L, **{name: _p((1 << 20) + 8)}) == E_ALIGN, name
        assert fn(L, seed=_p((1 << 20) + 4)) == E_ALIGN
    assert gd_fwd(L, y=A) == E_LAYOUT                       # y aliases h
    assert gd_bwd(L, dh=A) == E_LAYOUT and gd_bwd(L, dh=_p(3 << 20)) == E_LAYOUT


def aln_fwd(L, res=A, rdt=0, a=A, adt=1, rows=5, Cc=256, thr=6554, scale=1.1, seed=A, gamma=A, beta=A, s=B, y=B):
    return L.lss_add_dropout_ln_fwd(res, rdt, a, adt, rows, Cc, thr, scale, seed, gamma, beta, 1e-5, s, y, None)


def aln_bwd(L, s=A, dy=A, gdt=0, gamma=A, rows=5, Cc=256, thr=6554, scale=1.1, seed=A, ws=B, wsb=None, ds=B, da=B,
            adt=1, dg=B, db=B):
    if wsb is None:
        wsb = L.lss_add_dropout_ln_bwd_workspace_bytes(rows)
    return L.lss_add_dropout_ln_bwd(s, dy, gdt, gamma, rows, Cc, 1e-5, thr, scale, seed, ws, wsb, ds, da, adt, dg, db,
                                    None)


def test_add_dropout_ln_argument_checks(L):
    for name in ("res", "a", "gamma", "beta", "s", "y"):
        assert aln_fwd(L, **{name: None}) == E_NULL, name
    for name in ("s", "dy", "gamma", "ws", "ds", "da", "dg", "db"):
        assert aln_bwd(L, **{name: None}) == E_NULL, name
    for fn in (aln_fwd, aln_bwd):
        kw = dict(wsb=1 << 20) if fn is aln_bwd else {}
        assert fn(L, rows=0, **kw) == E_SHAPE and fn(L, rows=(1 << 22) + 1, **kw) == E_SHAPE
        assert fn(L, Cc=128) == E_SHAPE
        assert fn(L, thr=65536) == E_SHAPE and fn(L, thr=-1) == E_SHAPE
        assert fn(L, seed=_p((1 << 20) + 4)) == E_ALIGN
    for name in ("rdt", "adt"):
        assert aln_fwd(L, **{name: 2}) == E_LAYOUT and aln_fwd(L, **{name: -1}) == E_LAYOUT
    for name in ("gdt", "adt"):
        assert aln_bwd(L, **{name: 2}) == E_LAYOUT and aln_bwd(L, **{name: -1}) == E_LAYOUT
    for name in ("res", "a", "gamma", "beta", "s", "y"):
        assert aln_fwd(L, **{name: _p((1 << 20) + 8)}) == E_ALIGN, name
    for name in ("s", "dy", "gamma", "ws", "ds", "da"):
        assert aln_bwd(L, **{name: _p((1 << 20) + 8)}) == E_ALIGN, name
    assert aln_bwd(L, dg=_p((1 << 20) + 2)) == E_ALIGN and aln_bwd(L, db=_p((1 << 20) + 1)) == E_ALIGN
    assert aln_bwd(L, wsb=L.lss_add_dropout_ln_bwd_workspace_bytes(5) - 1) == E_WORKSPACE
    assert aln_bwd(L, wsb=0) == E_WORKSPACE


def test_threshold_rule():
    from lss2_multimodal_nu_amd import ops
    assert ops.dropout_threshold(0.0) == (0, 1.0)
    thr, scale = ops.dropout_threshold(0.1)
    assert thr == 6554 and scale == 1.0 / (1.0 - 6554 / 65536.0)
    assert ops.dropout_threshold(0.5) == (32768, 2.0)
    assert ops.dropout_threshold(65535.4 / 65536)[0] == 65535
    for p in (1.0, 0.999999, -0.1, 65535.6 / 65536):       # thr would be 65536: the torch composition's business
        assert ops.dropout_threshold(p) is None


def test_wrappers_reject_before_the_library(L):
    from lss2_multimodal_nu_amd import ops
    h = torch.zeros(4, 64).bfloat16()
    for kw in (dict(h=h.float()), dict(h=h[:, :32]), dict(h=torch.zeros(3, 4).bfloat16()), dict(seed=torch.zeros(2)),
               dict(seed=torch.zeros(3, dtype=torch.int64)), dict(p=1.0), dict()):   # the last: only the device is wrong
        a = dict(h=h, p=0.1, seed=torch.zeros(2, dtype=torch.int64))
        a.update(kw)
        with pytest.raises(ValueError):
            ops.gelu_dropout(a["h"], a["p"], a["seed"])
    for kw in (dict(dy=h.float()), dict(dy=h[:2]), dict()):
        a = dict(dy=h)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.gelu_dropout_bwd(h, a["dy"], 0.0, None)
    r, gamma = torch.zeros(3, 256), torch.ones(256)
    for kw in (dict(res=r.double()), dict(a=r.half()), dict(a=r[:2]), dict(res=torch.zeros(3, 128), a=torch.zeros(3, 128)),
               dict(gamma=torch.ones(128)), dict()):
        a = dict(res=r, a=r.bfloat16(), gamma=gamma)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.add_dropout_layernorm(a["res"], a["a"], a["gamma"], gamma, 1e-5)
    for kw in (dict(s=r.bfloat16()), dict(dy=r.half()), dict(dy=r[:2]), dict(da_dtype=torch.float16), dict()):
        a = dict(s=r, dy=r, da_dtype=torch.float32)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.add_dropout_layernorm_bwd(a["s"], a["dy"], gamma, 1e-5, a["da_dtype"])


def test_encoder_layer_on_cpu_tensors_takes_the_composition(monkeypatch):
    """bf16 autocast on the CPU: the K12 nodes are not used, `"pointwise"` does not advance, the torch composition runs
    and differentiates."""
    from lss2_multimodal_nu_amd import transformer_modules as tm
    monkeypatch.setenv("LSS_TRANSFORMER_NATIVE", "1")
    monkeypatch.setenv("LSS_TRANSFORMER_POINTWISE", "1")
    for fn in (tm._GeluDropoutFn, tm._AddDropoutLayerNormFn):
        monkeypatch.setattr(fn, "forward", lambda *a, **k: pytest.fail("native node used on CPU tensors"))
    torch.manual_seed(0)
    layer = tm.TransformerEncoderLayer(256, 8, 128, 0.1).train()
    src = torch.randn(1, 16, 256, requires_grad=True)
    pos = torch.randn(1, 256, 4, 4)
    ref = tm.LightweightBEVTransformer.reference_points(4, 4, "cpu")
    before = dict(tm.TRANSFORMER_CALLS)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out = layer(src, pos, ref)
    out.float().sum().backward()
    assert tm.TRANSFORMER_CALLS["composition"] == before["composition"] + 1
    assert tm.TRANSFORMER_CALLS["native"] == before["native"]
    assert tm.TRANSFORMER_CALLS["pointwise"] == before["pointwise"]
    assert src.grad is not None and layer.linear1.weight.grad is not None


def test_pointwise_route_conditions(monkeypatch):
    from torch import nn
    from lss2_multimodal_nu_amd import transformer_modules as tm
    monkeypatch.delenv("LSS_TRANSFORMER_POINTWISE", raising=False)
    layer = tm.TransformerEncoderLayer(256, 8, 128, 0.1)
    assert tm._pointwise_native_ok(layer) == (tm._TRANSFORMER_POINTWISE_DEFAULT != "0")
    monkeypatch.setenv("LSS_TRANSFORMER_POINTWISE", "1")
    assert tm._pointwise_native_ok(layer)
    assert tm._pointwise_native_ok(tm.TransformerEncoderLayer(256, 8, 128, 0.0))
    monkeypatch.setenv("LSS_TRANSFORMER_POINTWISE", "0")
    assert not tm._pointwise_native_ok(layer)
    monkeypatch.setenv("LSS_TRANSFORMER_POINTWISE", "1")
    layer.activation = nn.GELU(approximate="tanh")
    assert not tm._pointwise_native_ok(layer)
    layer.activation = nn.ReLU()
    assert not tm._pointwise_native_ok(layer)
    layer.activation = nn.GELU()
    layer.dropout2 = nn.Dropout(0.9999999)                 # no 16-bit threshold
    assert not tm._pointwise_native_ok(layer)


def test_kernels_use_no_scratch(tmp_path):
    """Resource usage of the gfx950 code of transformer_pointwise.hip from the compiler's metadata: no kernel has a
    private (scratch) segment or spills registers; only the backward's (2, 256) x 4 partial sums are in LDS."""
    import subprocess
    from lss2_multimodal_nu_amd import build_native
    asm = tmp_path / "transformer_pointwise.s"
    subprocess.check_call([build_native._hipcc(), "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(build_native.CSRC, "transformer_pointwise.hip")] + build_native.COMMON
                          + build_native.SOURCES["transformer_pointwise.hip"], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    kernels = [k for k in re.findall(r"\.name:\s+(\S+_kernel\S*)\n", text) if not k.endswith(".kd")]
    # 4 GELU forms, 8 row-forward forms, 8 + 8 forms of the one LayerNorm-backward template (plain and add-dropout),
    # its second stage
    assert len(kernels) == 29, kernels
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text))
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) in (0, 8192) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text))
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text and "atomic" not in text
