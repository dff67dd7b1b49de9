"""K15 on the GPU (csrc/txt_heads.hip).  Each launch alone against the fp64 reference at the DERIVED bounds of
tests/txt_heads_ref.py on every case (test_txt_heads_ref_cpu.py proves those bounds reject every planted defect);
strided inputs; bit-reproducible and independent of the batch.  Then the whole route on `compile_model_bevtxt`: taken
only behind LSS_TXT_HEADS_NATIVE=1 in eval / no-grad / bf16 / GPU, aware of parameter edits, capturable in one HIP
graph, and as close to the reference's outputs (g13_bevtxt_heads) as the library's own bf16 composition.  Every measured
error is `report`ed."""
import functools
import gc

import numpy as np
import pytest
import torch

import txt_heads_ref as R

pytestmark = pytest.mark.gpu

import lss2_multimodal_nu_amd as L  # noqa: E402
from lss2_multimodal_nu_amd import model_BEV_TXT as mb  # noqa: E402
from lss2_multimodal_nu_amd import ops  # noqa: E402
from oracle import vovnet_oracle as vo  # noqa: E402

GRID = dict(xbound=[-50.0, 50.0, 0.5], ybound=[-50.0, 50.0, 0.5], zbound=[-10.0, 10.0, 20.0], dbound=[4.0, 45.0, 1.0])
AUG = {"final_dim": (128, 352), "Ncams": 6}
POST_CASES = R.CASES + R.POST_EXTRA


# ----------------------------------------------------------------------------------------------------------------------
# the launches alone
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _post_case(name):
    c = {c.name: c for c in POST_CASES}[name]
    inputs = R.make_post_inputs(c)
    return c, inputs, R.ref_bev_post(inputs[0], c.origin, c.crop, *inputs[1:])


@functools.lru_cache(maxsize=None)
def _heads_case(name):
    c = R.BY_NAME[name]
    inputs = R.make_head_inputs(c)
    return c, inputs, R.ref_txt_heads(*inputs, c.cams, c.ncams)


def _run_post(c, inputs, m=None, origin=None):
    m0, w, sc, sh = inputs
    return ops.bev_post(m0.cuda() if m is None else m, c.origin if origin is None else origin, c.crop, w.cuda(), sc.cuda(),
                        sh.cuda())


def _gpu_set(hs):
    return (ops.pack_conv_weight(hs.w.cuda().contiguous(), ops.DT_BF16), hs.scale.cuda(), hs.shift.cuda(), hs.lin_w.cuda(),
            hs.lin_b.cuda())


def _run_heads(c, inputs, sample=None):
    scene, post, front, side, pred = inputs
    if sample is not None:
        scene, post = scene[sample * c.ncams:(sample + 1) * c.ncams], post[sample:sample + 1]
    return ops.txt_heads(scene.bfloat16().cuda().contiguous(), post.cuda().contiguous(), _gpu_set(front),
                         _gpu_set(side) if len(c.cams) > 1 else None, {k: v.cuda() for k, v in pred.items()}, c.cams, c.ncams)


@pytest.mark.parametrize("name", [c.name for c in POST_CASES])
def test_bev_post_against_fp64(name, report):
    c, inputs, ref = _post_case(name)
    got = _run_post(c, inputs)
    assert got.shape == (c.B, c.Cp, c.H, c.W) and got.dtype == torch.float32 and got.is_contiguous()
    e = R.check(got, ref.y, ref.bound, "bev_post " + name)
    report("txt_heads.bev_post.%s.max" % name, e[0])
    report("txt_heads.bev_post.%s.err_over_bound" % name, float(((got.double().cpu() - ref.y).abs() / ref.bound).max()))


@pytest.mark.parametrize("name", ["production", "partial_3x5", "pixel_1x1"])
def test_bev_post_reads_strided_views_in_place(name):
    """Channels-last memory, the crop handed over as a view (origin (0, 0)), and every second pixel of a larger map: the
    same values through other strides give the same bits."""
    c, inputs, _ = _post_case(name)
    m = inputs[0].cuda()
    want = _run_post(c, inputs)
    nhwc = m.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert nhwc.is_contiguous() == (c.Cb == 1) and torch.equal(_run_post(c, inputs, nhwc), want)
    (h0, w0), (Hc, Wc) = c.origin, c.crop
    for src in (m, nhwc):
        view = src[:, :, h0:h0 + Hc, w0:w0 + Wc]
        assert not view.is_contiguous() and torch.equal(_run_post(c, inputs, view, (0, 0)), want)
    big = torch.full((c.B, c.Cb, 2 * c.map[0], 2 * c.map[1]), 7.0, device="cuda")
    big[:, :, ::2, ::2] = m
    sparse = big[:, :, ::2, ::2]
    assert sparse.stride(3) == 2 and torch.equal(_run_post(c, inputs, sparse), want)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_txt_heads_against_fp64(name, report):
    c, inputs, ref = _heads_case(name)
    act, desc = _run_heads(c, inputs)
    assert act.shape == (c.B, c.n_act) and desc.shape == (c.B, c.n_desc_f + len(c.cams) - 1)
    assert act.dtype == desc.dtype == torch.float32
    for what, got, want, bound in (("act", act, ref.act, ref.bound_act), ("desc", desc, ref.desc, ref.bound_desc)):
        report("txt_heads.%s.%s.err_over_bound" % (name, what), float(((got.double().cpu() - want).abs() / bound).max()))
        e = R.check(got, want, bound, "%s %s" % (what, name))
        report("txt_heads.%s.%s.max" % (name, what), e[0])
        report("txt_heads.%s.%s.l2" % (name, what), e[1])


def test_bit_reproducible_and_batch_independent():
    c, inputs, _ = _heads_case("partial_3x5")
    assert c.B == 3
    a, b = _run_heads(c, inputs), _run_heads(c, inputs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i in range(c.B):
        alone = _run_heads(c, inputs, sample=i)
        assert all(torch.equal(x[0], y[i]) for x, y in zip(alone, a)), i
    c, inputs, _ = _heads_case("production")
    a = _run_heads(c, inputs)
    assert all(torch.equal(x, y) for x, y in zip(a, _run_heads(c, inputs)))
    assert all(torch.equal(x[0], y[1]) for x, y in zip(_run_heads(c, inputs, sample=1), a))
    c, pin, _ = _post_case("partial_3x5")
    p = _run_post(c, pin)
    assert torch.equal(p, _run_post(c, pin))
    for i in range(c.B):
        assert torch.equal(_run_post(c, pin, pin[0][i:i + 1].cuda())[0], p[i]), i


# ----------------------------------------------------------------------------------------------------------------------
# on the model
# ----------------------------------------------------------------------------------------------------------------------
def _fixture(golden):
    """g13_bevtxt_heads's `txt` state, x and bev exactly as test_modules_cpu.py loads them."""
    g = golden("g13_bevtxt_heads")
    keys = [str(k) for k in g["txt_keys"]]
    shapes = [tuple(int(d) for d in str(s).split(",")) if str(s) else () for s in g["txt_shapes"]]
    head = [(k, s) for k, s in zip(keys, shapes) if k.split(".")[0] not in ("dx", "bx", "nx", "frustum", "camencode")]
    state = vo.seeded_state(head, int(g["txt_seed"]))
    rs = np.random.RandomState
    B = int(g["B"])
    x = torch.from_numpy(rs(int(g["seed_x"])).randn(B * 6, 512, 8, 22).astype(np.float32))
    bev = torch.from_numpy(rs(int(g["seed_bev"])).randn(B, 4, 200, 200).astype(np.float32))
    return g, B, state, x, bev


def _model(golden, precision="bf16", device="cuda"):
    g, B, state, x, bev = _fixture(golden)
    m = L.compile_model_bevtxt(B, GRID, AUG, 4, precision=precision).eval()
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected
    m = m.to(device)
    x, bev = x.to(device), bev.to(device)
    m._bev = lambda *a: bev
    return m, x, bev, g


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    _post_case.cache_clear()
    _heads_case.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _forward(m, x, grad=False):
    with torch.set_grad_enabled(grad):
        return m(x, None, None, None, None, None)


def _expect(m, x, route, monkeypatch, why, grad=False):
    """One forward that must take `route`; K15 is wrapped so that the count is the kernel's, not only the counter's."""
    calls = []
    real = ops.txt_heads
    monkeypatch.setattr(ops, "txt_heads", lambda *a, **k: calls.append(1) or real(*a, **k))
    before = dict(mb.TXT_HEADS_CALLS)
    out = _forward(m, x, grad)
    monkeypatch.setattr(ops, "txt_heads", real)
    other = "composition" if route == "native" else "native"
    assert mb.TXT_HEADS_CALLS == {route: before[route] + 1, other: before[other]}, why
    assert len(calls) == (1 if route == "native" else 0), why
    return out


def test_route_is_taken_only_where_documented(golden, monkeypatch):
    import warnings
    m, x, bev, _ = _model(golden)
    monkeypatch.delenv("LSS_TXT_HEADS_NATIVE", raising=False)
    lib = _expect(m, x, "composition", monkeypatch, "switch unset")
    monkeypatch.setenv("LSS_TXT_HEADS_NATIVE", "1")
    bev_o, act, desc = _expect(m, x, "native", monkeypatch, "open")
    assert bev_o is bev and act.shape == (x.shape[0] // 6, 4) and desc.shape == (x.shape[0] // 6, 8)
    assert act.dtype == desc.dtype == torch.float32
    # the bf16 scene map is a few 1e-3 from the fp32 heads, not more
    assert float((act - lib[1]).abs().max()) < 0.05 * float(lib[1].abs().max())
    assert float((desc - lib[2]).abs().max()) < 0.05 * float(lib[2].abs().max())
    monkeypatch.setenv("LSS_TXT_HEADS_NATIVE", "0")
    _expect(m, x, "composition", monkeypatch, "switch 0")
    monkeypatch.setenv("LSS_TXT_HEADS_NATIVE", "1")
    m.embeder_lr1.train()
    _expect(m, x, "composition", monkeypatch, "train")
    m.eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = _expect(m, x, "composition", monkeypatch, "autograd", grad=True)
    assert out[1].requires_grad
    seen = []
    hook = m.embeder_f1.register_forward_hook(lambda mod, args, out: seen.append(out))
    _expect(m, x, "composition", monkeypatch, "hook")
    hook.remove()
    assert len(seen) == 1
    _expect(m, x, "native", monkeypatch, "open again")
    kept = m.sceneunder
    m.sceneunder = torch.nn.Sequential(torch.nn.Conv2d(512, 256, 1)).cuda().eval()
    _expect(m, x, "composition", monkeypatch, "replaced sceneunder")
    m.sceneunder = kept
    _expect(m, x, "native", monkeypatch, "put back")
    m32, x32, _, _ = _model(golden, precision="fp32")
    _expect(m32, x32, "composition", monkeypatch, "fp32 precision")
    mc, xc, _, _ = _model(golden, device="cpu")
    _expect(mc, xc, "composition", monkeypatch, "cpu")


def test_parameter_edits_are_seen(golden, monkeypatch):
    monkeypatch.setenv("LSS_TXT_HEADS_NATIVE", "1")
    m, x, _, _ = _model(golden)
    _, a0, d0 = _expect(m, x, "native", monkeypatch, "start")
    with torch.no_grad():
        m.predictorlr[0].bias.add_(0.5)
    _, a1, d1 = _expect(m, x, "native", monkeypatch, "bias edit")
    assert torch.equal(a0, a1) and torch.equal(d0[:, :4], d1[:, :4])
    assert float((d1[:, 4:] - d0[:, 4:] - 0.5).abs().max()) < 1e-6
    with torch.no_grad():
        m.embeder_f1[1].weight.mul_(1.5)                    # a folded BatchNorm is refolded
    _, a2, d2 = _expect(m, x, "native", monkeypatch, "bn edit")
    assert not torch.equal(a1, a2) and torch.equal(d1[:, 4:], d2[:, 4:])
    sd = {k: v.clone() for k, v in m.embeder_lr2.state_dict().items()}
    sd["1.bias"] += 1.0
    m.embeder_lr2.load_state_dict(sd)
    _, a3, d3 = _expect(m, x, "native", monkeypatch, "load_state_dict")
    assert torch.equal(a2, a3) and not torch.equal(d2[:, 4:], d3[:, 4:])


def test_graph_capture_of_the_txt_half(golden, monkeypatch):
    monkeypatch.setenv("LSS_TXT_HEADS_NATIVE", "1")
    m, x, bev, _ = _model(golden)
    crop = bev[:, :, 60:140, 56:144]
    xs = [x, x.flip(0).contiguous(), (x * 0.5).contiguous()]
    with torch.no_grad():
        eager = [tuple(t.clone() for t in m._txt_heads(xi, crop)) for xi in xs]
        buf = x.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m._txt_heads(buf, crop)                           # warm-up on the capture stream: allocator and caches primed
        torch.cuda.current_stream().wait_stream(s)
        before = mb.TXT_HEADS_CALLS["native"]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m._txt_heads(buf, crop)
        assert mb.TXT_HEADS_CALLS["native"] == before + 1
    for xi, want in zip(xs, eager):
        buf.copy_(xi)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, want))


def test_reference_parity_against_the_librarys_bf16(golden, monkeypatch, report):
    """The native act / desc lie no further from the reference's own outputs (the fixture) than TWICE the error of
    torch's bf16-autocast composition of the same modules on the same inputs, in max-abs and rel-L2: the autocast
    composition, not the code under test, sets the bar (K13's precedent for "as good as the library's bf16")."""
    m, x, bev, g = _model(golden)
    want = {"act": torch.from_numpy(g["txt_act"]), "desc": torch.from_numpy(g["txt_desc"])}
    monkeypatch.setenv("LSS_TXT_HEADS_NATIVE", "1")
    _, act, desc = _expect(m, x, "native", monkeypatch, "native")
    monkeypatch.delenv("LSS_TXT_HEADS_NATIVE")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        lib_act, lib_desc = m._txt_heads(x, bev[:, :, 60:140, 56:144])
    _, f32_act, f32_desc = _expect(m, x, "composition", monkeypatch, "fp32 composition")
    for name, nat, lib, f32 in (("act", act, lib_act, f32_act), ("desc", desc, lib_desc, f32_desc)):
        en, el, ef = R.errors(nat, want[name]), R.errors(lib.float(), want[name]), R.errors(f32, want[name])
        for k, i in (("max", 0), ("l2", 1)):
            report("txt_heads.parity.%s.native.%s" % (name, k), en[i])
            report("txt_heads.parity.%s.autocast.%s" % (name, k), el[i])
            report("txt_heads.parity.%s.fp32.%s" % (name, k), ef[i])
        print("parity %s: native %.3e / %.3e  autocast %.3e / %.3e  fp32 %.3e / %.3e" % ((name,) + en + el + ef))
        assert en[0] <= 2 * el[0] and en[1] <= 2 * el[1], (name, en, el)
