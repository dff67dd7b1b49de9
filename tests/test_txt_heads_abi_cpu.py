"""K15 without a GPU: the header, `_native.SIGNATURES` and the library agree on the four entries and the descriptor;
`lss_txt_heads_ok`'s truth table and the workspace size; every refusal code of the two launchers on addresses that are
never dereferenced (all checks run before any HIP call) with the output buffers left as they were; the `ValueError`s of
the ops wrappers; the routing of `BEV_TXT._txt_heads` to the library composition; and the resource usage of the gfx950
code."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import lss2_multimodal_nu_amd as L_
from lss2_multimodal_nu_amd import _native as N
from lss2_multimodal_nu_amd import build_native, ops
from lss2_multimodal_nu_amd import model_BEV_TXT as mb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_LAYOUT, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4, -5
ENTRIES = ("lss_bev_post_fwd", "lss_txt_heads_ok", "lss_txt_heads_workspace_bytes", "lss_txt_heads_fwd")
GRID = dict(xbound=[-50.0, 50.0, 0.5], ybound=[-50.0, 50.0, 0.5], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
AUG = {"final_dim": (128, 352), "Ncams": 6}


@pytest.fixture(scope="module")
def L():
    build_native.build(verbose=False)
    return N.lib()


def _header():
    return open(os.path.join(ROOT, "include", "lss_hip.h")).read()


def test_header_signatures_and_library_agree(L):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name + " is not declared in include/lss_hip.h"
        params = [p.strip() for p in m.group(2).split(",")]
        res, args = N.SIGNATURES[name]
        assert res is (ctypes.c_int if m.group(1) == "int" else ctypes.c_size_t) and len(args) == len(params), name
        for p, a in zip(params, args):
            assert (a is ctypes.c_void_p) == ("*" in p), (name, p)
            assert (a is ctypes.c_longlong) == ("long long" in p and "*" not in p), (name, p)
        assert hasattr(L, name)
    assert "csrc/txt_heads.hip" in _header() and "txt_heads.hip" in build_native.SOURCES
    assert re.search(r"K15.*?replaces: src/modules\.py:133-144 and src/model_BEV_TXT\.py:285-287.*?"
                     r"src/model_BEV_TXT\.py:293-332", _header(), flags=re.S)


def test_struct_matches_the_header():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, code, flags=re.S).group(1)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            kind = "ptr" if "*" in decl else decl.split()[0]
            for n in decl.split(",") if kind in ("ptr", "int32_t") else [decl]:
                out.append((n.split()[-1].strip("* "), kind))
        return out

    assert fields("lss_txt_heads_set") == [(f[0], "ptr") for f in N.TxtHeadsSet._fields_]
    want = {ctypes.c_void_p: "ptr", ctypes.c_int32: "int32_t", ctypes.c_uint64: "uint64_t", N.TxtHeadsSet: "lss_txt_heads_set_t",
            ctypes.c_int32 * 8: "int32_t"}
    got = fields("lss_txt_heads_desc")
    # `front, side` is one declaration of two sets; `cams[8]` one array
    names = [n for n, _ in got]
    assert names == ["scene", "bev_post", "side", "f1_w", "f1_b", "f2_w", "f2_b", "lr_w", "lr_b", "workspace", "act",
                     "desc", "workspace_bytes", "cams[8]", "B", "ncams", "n_slots", "H", "W", "Cp", "E", "n_act",
                     "n_desc_f", "reserved"]
    mine = [(f[0], want[f[1]]) for f in N.TxtHeadsDesc._fields_ if f[0] != "front"]
    assert [(n.replace("[8]", ""), k) for n, k in got] == mine
    assert re.search(r"lss_txt_heads_set_t front, side;", code)
    assert ctypes.sizeof(N.TxtHeadsSet) == 40
    assert ctypes.sizeof(N.TxtHeadsDesc) == 2 * 8 + 2 * 40 + 9 * 8 + 8 + 8 * 4 + 10 * 4


def test_ok_truth_table_and_workspace(L):
    ok, ws = L.lss_txt_heads_ok, L.lss_txt_heads_workspace_bytes
    good = (4, 6, 5, 8, 22, 8, 40, 4, 4)
    for args in (good, (1, 1, 1, 1, 1, 1, 1, 1, 1), (65535, 64, 8, 256, 256, 8, 64, 16, 16), (3, 6, 5, 3, 5, 5, 40, 4, 4)):
        assert ok(*args) == 1 and ops.txt_heads_ok(*args), args
    for i, bad in ((0, 0), (0, 65536), (1, 0), (1, 65), (2, 0), (2, 9), (3, 0), (3, 1025), (4, 0), (4, 1025), (5, 0), (5, 9),
                   (6, 0), (6, 65), (7, 0), (7, 17), (8, 0), (8, 17), (0, -1)):
        args = list(good)
        args[i] = bad
        assert ok(*args) == E_SHAPE and not ops.txt_heads_ok(*args), args
    assert ok(1, 6, 5, 512, 512, 8, 40, 4, 4) == E_SHAPE         # H W > 65536
    # B x slots x ceil(HW / 16) x E floats; proportional to B: a sample's tiles do not depend on its batch
    assert ws(4, 5, 8, 22, 40) == 4 * 5 * 11 * 40 * 4
    assert ws(1, 5, 8, 22, 40) * 7 == ws(7, 5, 8, 22, 40)
    assert ws(3, 5, 3, 5, 40) == 3 * 5 * 1 * 40 * 4 and ws(2, 1, 5, 7, 64) == 2 * 1 * 3 * 64 * 4
    assert ws(2, 5, 1, 1, 7) == 2 * 5 * 7 * 4
    assert ws(0, 5, 8, 22, 40) == 0 and ws(1, 9, 8, 22, 40) == 0 and ws(1, 5, 8, 22, 65) == 0 and ws(1, 5, 0, 22, 40) == 0


PATTERN = b"\xa5" * 4096


def _desc(out, **kw):
    """A launch every check accepts, on addresses nothing dereferences - but for the outputs and the workspace, which are
    host buffers holding a pattern; `kw` overrides fields (a.b for the sets)."""
    d = N.TxtHeadsDesc()
    i = 1
    for name in ("scene", "bev_post") + N.TxtHeadsDesc.PREDICTORS:
        setattr(d, name, 4096 * i)
        i += 1
    for s in (d.front, d.side):
        for f, _ in N.TxtHeadsSet._fields_:
            setattr(s, f, 4096 * i)
            i += 1
    d.workspace, d.act, d.desc = (ctypes.addressof(b) for b in out)
    d.B, d.ncams, d.n_slots, d.H, d.W, d.Cp, d.E, d.n_act, d.n_desc_f = 1, 6, 5, 2, 3, 8, 40, 4, 4
    d.workspace_bytes = 1 * 5 * 1 * 40 * 4
    for s, c in enumerate((1, 0, 3, 2, 5)):
        d.cams[s] = c
    for k, v in kw.items():
        if k.startswith("cam_"):
            d.cams[int(k[4:])] = v
        elif "." in k:
            setattr(getattr(d, k.split(".")[0]), k.split(".")[1], v)
        else:
            setattr(d, k, v)
    return d


HEADS_REFUSALS = [
    ("scene_null", dict(scene=None), E_NULL),
    ("bev_post_null", dict(bev_post=None), E_NULL),
    ("front_weight_null", {"front.embed_w": None}, E_NULL),
    ("front_linear_null", {"front.lin_w": None}, E_NULL),
    ("side_shift_null", {"side.embed_shift": None}, E_NULL),
    ("side_bias_null", {"side.lin_b": None}, E_NULL),
    ("f1_null", dict(f1_w=None), E_NULL),
    ("f2_bias_null", dict(f2_b=None), E_NULL),
    ("lr_null", dict(lr_w=None), E_NULL),
    ("workspace_null", dict(workspace=None), E_NULL),
    ("act_null", dict(act=None), E_NULL),
    ("desc_null", dict(desc=None), E_NULL),
    ("b_0", dict(B=0), E_SHAPE),
    ("b_65536", dict(B=65536), E_SHAPE),
    ("ncams_0", dict(ncams=0), E_SHAPE),
    ("slots_0", dict(n_slots=0), E_SHAPE),
    ("slots_9", dict(n_slots=9), E_SHAPE),
    ("h_0", dict(H=0), E_SHAPE),
    ("w_1025", dict(W=1025), E_SHAPE),
    ("cp_0", dict(Cp=0), E_SHAPE),
    ("cp_9", dict(Cp=9), E_SHAPE),
    ("e_65", dict(E=65), E_SHAPE),
    ("act_classes_17", dict(n_act=17), E_SHAPE),
    ("desc_classes_0", dict(n_desc_f=0), E_SHAPE),
    ("camera_6_of_6", dict(cam_4=6), E_SHAPE),
    ("camera_negative", dict(cam_0=-1), E_SHAPE),
    ("scene_unaligned", dict(scene=4096 + 8), E_ALIGN),
    ("front_image_unaligned", {"front.embed_w": 4096 * 20 + 8}, E_ALIGN),
    ("side_image_unaligned", {"side.embed_w": 4096 * 30 + 4}, E_ALIGN),
    ("linear_unaligned", {"side.lin_w": 4096 * 30 + 2}, E_ALIGN),
    ("scale_unaligned", {"front.embed_scale": 4096 * 20 + 1}, E_ALIGN),
    ("bev_post_unaligned", dict(bev_post=4096 + 2), E_ALIGN),
    ("predictor_unaligned", dict(lr_b=4096 + 3), E_ALIGN),
    ("workspace_short", dict(workspace_bytes=1 * 5 * 1 * 40 * 4 - 1), E_WORKSPACE),
    ("workspace_for_a_smaller_batch", dict(B=2), E_WORKSPACE),
]


@pytest.mark.parametrize("what,fields,code", HEADS_REFUSALS, ids=[r[0] for r in HEADS_REFUSALS])
def test_heads_refusals_leave_the_outputs_alone(L, what, fields, code):
    out = [ctypes.create_string_buffer(PATTERN, len(PATTERN)) for _ in range(3)]
    assert L.lss_txt_heads_fwd(ctypes.byref(_desc(out, **fields)), None) == code
    assert all(b.raw == PATTERN for b in out)
    assert L.lss_error_string(code)


def test_heads_refusals_one_slot(L):
    out = [ctypes.create_string_buffer(PATTERN, len(PATTERN)) for _ in range(3)]
    assert L.lss_txt_heads_fwd(None, None) == E_NULL
    # with one slot the side set and lr are not looked at, the rest still is
    side = {"side." + f: None for f, _ in N.TxtHeadsSet._fields_}
    one = dict(side, lr_w=None, lr_b=None, n_slots=1)
    assert L.lss_txt_heads_fwd(ctypes.byref(_desc(out, **dict(one, E=65))), None) == E_SHAPE
    assert L.lss_txt_heads_fwd(ctypes.byref(_desc(out, **dict(one, f1_b=4100 + 1))), None) == E_ALIGN
    assert L.lss_txt_heads_fwd(ctypes.byref(_desc(out, **dict(one, scene=None))), None) == E_NULL
    assert L.lss_txt_heads_fwd(ctypes.byref(_desc(out, **dict(one, workspace_bytes=159))), None) == E_WORKSPACE
    assert L.lss_txt_heads_fwd(ctypes.byref(_desc(out, **dict(one, cam_0=7))), None) == E_SHAPE
    assert all(b.raw == PATTERN for b in out)


def test_bev_post_refusals(L):
    y = ctypes.create_string_buffer(PATTERN, len(PATTERN))
    p = ctypes.c_void_p
    #        x        sb      sc   sh  sw Hm  Wm  h0 w0 B Cb Hc  Wc  w        scale    shift    Co y                     stream
    good = [p(4096), 16000, 4000, 50, 1, 80, 50, 5, 7, 2, 4, 30, 20, p(8192), p(12288), p(16384), 8, p(ctypes.addressof(y)), None]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.lss_bev_post_fwd(*a)

    for i in (0, 13, 14, 15, 17):
        assert call(**{"a%d" % i: None}) == E_NULL, i
    for i, v in ((9, 0), (9, 65536), (10, 0), (10, 9), (16, 0), (16, 17), (11, 0), (12, 0), (7, -1), (8, -1), (5, 0), (6, 0),
                 (7, 51), (8, 31),       # the crop leaves the map
                 (11, 8), (12, 3)):      # no complete pool window: Ho = 0, Wo = 0
        assert call(**{"a%d" % i: v}) == E_SHAPE, (i, v)
    for i in (1, 2, 3, 4):
        assert call(**{"a%d" % i: -1}) == E_LAYOUT, i
    for i in (0, 13, 14, 15):
        assert call(**{"a%d" % i: p(4096 * (i + 1) + 2)}) == E_ALIGN, i
    assert call(a17=p(ctypes.addressof(y) + 2)) == E_ALIGN
    assert y.raw == PATTERN


def test_wrapper_value_errors():
    bev = torch.zeros(2, 4, 40, 30)
    w, sc, sh = torch.zeros(8, 4, 3, 3), torch.ones(8), torch.zeros(8)
    with pytest.raises(ValueError):                # CPU tensors never reach the library
        ops.bev_post(bev, (5, 7), (30, 20), w, sc, sh)
    with pytest.raises(ValueError):
        ops.bev_post(bev.double(), (5, 7), (30, 20), w, sc, sh)
    with pytest.raises(ValueError):
        ops.bev_post(bev[0], (5, 7), (30, 20), w, sc, sh)
    scene = torch.zeros(12, 3, 5, 256, dtype=torch.bfloat16)
    post = torch.zeros(2, 8, 3, 5)
    K = 40 * 15
    st = (torch.zeros(9, 32, 256, dtype=torch.bfloat16), torch.ones(32), torch.zeros(32), torch.zeros(40, K), torch.zeros(40))
    pred = {"f1_w": torch.zeros(4, 40), "f1_b": torch.zeros(4), "f2_w": torch.zeros(4, 40), "f2_b": torch.zeros(4),
            "lr_w": torch.zeros(1, 40), "lr_b": torch.zeros(1)}
    for bad in (scene, scene.float(), scene[:, :, :, ::2], scene[0]):
        with pytest.raises(ValueError):
            ops.txt_heads(bad, post, st, st, pred)


def _model():
    torch.manual_seed(0)
    return L_.compile_model_bevtxt(2, GRID, AUG, 4).eval()


def test_everything_but_the_open_route_takes_the_composition(monkeypatch):
    """Without a GPU nothing can open the route: the switch set or not, `_txt_heads` is the composition it was, counted,
    and K15 is never asked."""
    monkeypatch.setattr(ops, "txt_heads", lambda *a, **k: pytest.fail("K15 used"))
    monkeypatch.setattr(ops, "bev_post", lambda *a, **k: pytest.fail("K15's BevPost used"))
    m = _model()
    x, bev = torch.randn(12, 512, 8, 22), torch.randn(2, 4, 200, 200)
    m._bev = lambda *a: bev
    assert os.environ.get("LSS_TXT_HEADS_NATIVE") is None and mb._TXT_HEADS_NATIVE_DEFAULT == "0"
    outs = []
    for switch in (None, "1", "0"):
        if switch is not None:
            monkeypatch.setenv("LSS_TXT_HEADS_NATIVE", switch)
        before = dict(mb.TXT_HEADS_CALLS)
        with torch.no_grad():
            outs.append(m(x, None, None, None, None, None))
        assert mb.TXT_HEADS_CALLS == {"native": before["native"], "composition": before["composition"] + 1}, switch
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o, outs[0]))
    assert outs[0][1].shape == (2, 4) and outs[0][2].shape == (2, 8)


def test_plan_reads_structure_mode_and_hooks():
    m = _model()
    P = mb._TxtHeadsPlan
    mods = P.modules_of(m)
    assert mods is not None and m.embeder_f1[0] in mods and m.bevpost.post[0] in mods and m.sceneunder[0].project[0] in mods
    plan = P(m)
    assert plan.current(m) and plan.quiet()
    for target in (m.embeder_f1, m.sceneunder[0].convs[2][0], m.predictorlr[0], m.bevpost):
        for reg in ("register_forward_hook", "register_forward_pre_hook"):
            h = getattr(target, reg)(lambda *a: None)
            assert not plan.quiet(), (target, reg)
            h.remove()
            assert plan.quiet()
    h = torch.nn.modules.module.register_module_forward_hook(lambda *a: None)
    assert not plan.quiet()
    h.remove()
    m.embeder_lr2.train()
    assert not plan.quiet()
    m.eval()
    nn = torch.nn
    foreign = [
        ("replaced sceneunder", lambda m: setattr(m, "sceneunder", nn.Sequential(nn.Conv2d(512, 256, 1)))),
        ("four atrous rates", lambda m: setattr(m, "sceneunder", nn.Sequential(L_.heads.ASPP(512, [6, 12, 18, 24])))),
        ("embedder with a bias", lambda m: m.embeder_f1.__setitem__(0, nn.Conv2d(256, 32, 3, padding=1))),
        ("embedder 5x5", lambda m: m.embeder_lr1.__setitem__(0, nn.Conv2d(256, 32, 5, padding=2, bias=False))),
        ("embedder 64 wide", lambda m: setattr(m, "embeder_f1", L_.heads.Embedder_f1(256, 64))),
        ("gelu", lambda m: m.embeder_f1.__setitem__(2, nn.GELU())),
        ("linear without bias", lambda m: m.embeder_f2.__setitem__(1, nn.Linear(7040, 40, bias=False))),
        ("two linear widths", lambda m: m.embeder_lr2.__setitem__(1, nn.Linear(7040, 48))),
        ("two side classes", lambda m: setattr(m, "predictorlr", L_.heads.Predictor(40, 2))),
        ("deeper predictor", lambda m: setattr(m, "predictorf1", nn.Sequential(nn.Linear(40, 40), nn.Linear(40, 4)))),
        ("BevPost stride 2", lambda m: m.bevpost.post.__setitem__(0, nn.Conv2d(4, 8, 3, stride=2, padding=1, bias=False))),
        ("BevPost average pool", lambda m: m.bevpost.post.__setitem__(3, nn.AvgPool2d((5, 4)))),
        ("BevPost pool stride", lambda m: m.bevpost.post.__setitem__(3, nn.MaxPool2d((5, 4), stride=(5, 2)))),
    ]
    for why, edit in foreign:
        f = _model()
        assert P.modules_of(f) is not None
        edit(f)
        assert P.modules_of(f) is None, why
    m.predictorf2 = L_.heads.Predictor(40, 4).eval()     # a replaced module makes the plan stale
    assert not plan.current(m) and P.modules_of(m) is not None


def test_kernels_use_no_scratch(tmp_path):
    """Resource usage of the gfx950 code of txt_heads.hip: no private segment, no spills, LDS within 64 KiB, no atomics."""
    asm = tmp_path / "txt_heads.s"
    subprocess.check_call([build_native._hipcc(), "-S", "--cuda-device-only", "-o", str(asm),
                           os.path.join(build_native.CSRC, "txt_heads.hip")] + build_native.COMMON
                          + build_native.SOURCES["txt_heads.hip"], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    kernels = [k for k in re.findall(r"\.name:\s+(\S*(?:bev_post|txt_heads_tile|txt_heads_sum)_kernel\S*)\n", text)
               if not k.endswith(".kd")]
    assert len(kernels) == 3, kernels
    assert [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)] == [0, 0, 0]
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text))
    assert all(int(v) == 0 for v in re.findall(r"\.sgpr_spill_count:\s*(\d+)", text))
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", text)]
    assert len(lds) == 3 and all(v <= 64 * 1024 for v in lds)
    assert "global_atomic" not in text and "flat_atomic" not in text and "ds_add_f32" not in text
    assert text.count("v_mfma_f32_16x16x32_bf16") >= 36    # nine taps x four K blocks in the tile kernel
