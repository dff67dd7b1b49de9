"""The three host routes to the forward conv kernels give the same bits: an `ops` wrapper called eagerly (one
lss_conv_launch_t through lss_conv2d_sequence), the same call recorded and replayed by `ops.ConvPlan`, and the matching
lss_conv2d_*_fwd entry of the C ABI called positionally - for every kind of launch descriptor, at the smallest shapes
each kernel family takes.  What the kernels compute is checked against torch elsewhere (test_kernels_gpu.py,
test_conv_ks*_gpu.py, test_conv_ring_gpu.py); here only the routes are compared, so the comparison is exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from lss2_multimodal_nu_amd import ops as _ops
    return _ops


def _rand(gen, *shape, dtype=torch.bfloat16, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).cuda().to(dtype).contiguous()


def _weight(gen, Cout, Cin, K):
    return (torch.randn(Cout, Cin, K, K, generator=gen) * (Cin * K * K) ** -0.5).cuda()


def _bn(gen, n):
    return (torch.rand(n, generator=gen) + 0.5).cuda(), (torch.randn(n, generator=gen) * 0.1).cuda()


# Every case returns (x, wrapper, entry): `wrapper()` calls ops and returns the output(s); `entry(*outs)` calls the ABI
# entry positionally, writing into tensors shaped like the wrapper's outputs.  x is the tensor a plan is keyed on.

def _k0_plain(ops, gen, Cout):
    L, p = ops.N.lib(), ops.N.ptr
    x, res = _rand(gen, 1, 16, 16, 64), _rand(gen, 1, 16, 16, Cout)
    w = ops.pack_conv_weight(_weight(gen, Cout, 64, 3), ops.DT_BF16)
    sc, sh = _bn(gen, Cout)
    return (x, lambda: ops.conv2d_nhwc(x, w, (3, 3), 1, 1, sc, sh, res, True),
            lambda y: L.lss_conv2d_fwd(p(x), None, p(w), p(sc), p(sh), p(res), p(y), None, 1, 16, 16, 64, 0, 1, Cout,
                                       3, 3, 1, 1, ops.ACT_RELU, ops.DT_BF16, ops.N.stream()))


def _k0_fused_up2(ops, gen):
    L, p = ops.N.lib(), ops.N.ptr
    x, x2 = _rand(gen, 1, 8, 8, 64), _rand(gen, 1, 16, 16, 64)
    w = ops.pack_conv_weight(_weight(gen, 128, 128, 3), ops.DT_BF16)
    sc, sh = _bn(gen, 128)
    return (x, lambda: ops.conv2d_nhwc(x, w, (3, 3), 1, 1, sc, sh, None, True, x2=x2, up=2),
            lambda y: L.lss_conv2d_fwd(p(x), p(x2), p(w), p(sc), p(sh), None, p(y), None, 1, 8, 8, 64, 64, 2, 128,
                                       3, 3, 1, 1, ops.ACT_RELU, ops.DT_BF16, ops.N.stream()))


def _k0_1x1_gelu_f32(ops, gen):
    L, p = ops.N.lib(), ops.N.ptr
    x = _rand(gen, 1, 16, 16, 64)
    w = ops.pack_conv_weight(_weight(gen, 64, 64, 1), ops.DT_BF16)
    sh = _bn(gen, 64)[1]
    return (x, lambda: ops.conv2d_nhwc(x, w, (1, 1), 1, 0, None, sh, None, ops.ACT_GELU, out_f32=True),
            lambda y: L.lss_conv2d_fwd(p(x), None, p(w), None, p(sh), None, p(y), None, 1, 16, 16, 64, 0, 1, 64,
                                       1, 1, 1, 0, ops.ACT_GELU | ops.OUT_F32, ops.DT_BF16, ops.N.stream()))


def _k0_fp32(ops, gen):
    L, p = ops.N.lib(), ops.N.ptr
    x = _rand(gen, 1, 16, 16, 8, dtype=torch.float32)
    w = ops.pack_conv_weight(_weight(gen, 8, 8, 3), ops.DT_F32)
    return (x, lambda: ops.conv2d_nhwc(x, w, (3, 3), 1, 1, dt=ops.DT_F32),
            lambda y: L.lss_conv2d_fwd(p(x), None, p(w), None, None, None, p(y), None, 1, 16, 16, 8, 0, 1, 8,
                                       3, 3, 1, 1, ops.ACT_NONE, ops.DT_F32, ops.N.stream()))


def _k0_ks(ops, gen):
    """The smallest shape of tests/test_conv_ks_gpu.py (EXACT_SHAPES)."""
    L, p = ops.N.lib(), ops.N.ptr
    B, H, W, Cin, Cout = 3, 23, 21, 256, 128
    assert ops.conv_ks_ok(B, H, W, Cin, Cout)
    x, res = _rand(gen, B, H, W, Cin), _rand(gen, B, H, W, Cout)
    w = ops.pack_conv_weight_ks(_weight(gen, Cout, Cin, 3))
    sc, sh = _bn(gen, Cout)
    return (x, lambda: ops.conv2d_nhwc(x, w, (3, 3), 1, 1, sc, sh, res, True),
            lambda y: L.lss_conv2d_fwd(p(x), None, p(w.data), p(sc), p(sh), p(res), p(y), None, B, H, W, Cin, 0, 1,
                                       Cout, 3, 3, 1, 1, ops.ACT_RELU | ops.W_KS, ops.DT_BF16, ops.N.stream()))


def _k0_ring(ops, gen):
    """The smallest shape of tests/test_conv_ring_gpu.py (SHAPES): a x4 upsample of an odd-sized source."""
    L, p = ops.N.lib(), ops.N.ptr
    B, H, W, Cx, Cout, up = 10, 13, 27, 96, 128, 4
    assert ops.conv_ring_ok(B, H, W, Cx, 0, up, Cout, 0)
    x = _rand(gen, B, H, W, Cx)
    w = ops.pack_conv_weight_ring(_weight(gen, Cout, Cx, 3))
    sc, sh = _bn(gen, Cout)
    return (x, lambda: ops.conv2d_nhwc(x, w, (3, 3), 1, 1, sc, sh, None, True, None, up),
            lambda y: L.lss_conv2d_fwd(p(x), None, p(w.data), p(sc), p(sh), None, p(y), None, B, H, W, Cx, 0, up,
                                       Cout, 3, 3, 1, 1, ops.ACT_RELU | ops.W_RING, ops.DT_BF16, ops.N.stream()))


def _k1(ops, gen, K):
    L, p = ops.N.lib(), ops.N.ptr
    x, res = _rand(gen, 1, 16, 16, 64), _rand(gen, 1, 8, 8, 64)
    w32 = _weight(gen, 64, 64, K)
    w = ops.pack_conv_weight(w32, ops.DT_BF16) if K == 1 else ops.pack_conv_weight_s2d(w32, K // 2)
    sc, sh = _bn(gen, 64)
    return (x, lambda: ops.conv2d_s2_nhwc(x, w, K, K // 2, sc, sh, res, True),
            lambda y: L.lss_conv2d_s2_fwd(p(x), p(w), p(sc), p(sh), p(res), p(y), None, 1, 16, 16, 64, 64, K, K // 2,
                                          1, ops.N.stream()))


def _k2(ops, gen, B, H, W, Cx, Cout, up, n, ring=False):
    L, p = ops.N.lib(), ops.N.ptr
    x = _rand(gen, B, H, W, Cx)
    w32 = _weight(gen, Cout, Cx, 3)
    w = ops.pack_conv_weight_ring(w32) if ring else ops.pack_conv_weight(w32, ops.DT_BF16)
    sc, sh = _bn(gen, Cout)
    hw, hb = (torch.randn(n, Cout, generator=gen) * Cout ** -0.5).cuda(), torch.randn(n, generator=gen).cuda()
    return (x, lambda: ops.conv3x3_head_nchw(x, w, sc, sh, hw, hb, up=up),
            lambda out: L.lss_conv2d_head_fwd(p(x), None, p(w.data if ring else w), p(sc), p(sh), p(hw), p(hb), p(out),
                                              B, H, W, Cx, 0, up, Cout, n, 1 | (ops.W_RING if ring else 0),
                                              ops.N.stream()))


def _k2_ring(ops, gen):
    """A head case of tests/test_conv_ring_gpu.py: a wide, flat image, x2 upsample, 2-class head."""
    assert ops.conv_ring_ok(10, 7, 100, 64, 0, 2, 128, 2)
    return _k2(ops, gen, 10, 7, 100, 64, 128, 2, 2, ring=True)


def _k3(ops, gen):
    L, p = ops.N.lib(), ops.N.ptr
    x = _rand(gen, 1, 16, 16, 64)
    w = ops.pack_conv_weight_s2d(_weight(gen, 256, 64, 3), 1)
    sc, sh = _bn(gen, 256)
    return (x, lambda: ops.conv2d_s2_dual_nhwc(x, w, sc, sh, 128),
            lambda y, y2: L.lss_conv2d_s2_dual_fwd(p(x), p(w), p(sc), p(sh), p(y), p(y2), 1, 16, 16, 64, 256, 128, 3,
                                                   1, 1, ops.N.stream()))


def _k4(ops, gen):
    """The smallest shape of tests/test_conv_ks_s2_gpu.py (EXACT_SHAPES)."""
    L, p = ops.N.lib(), ops.N.ptr
    B, H, W, Cin, Cout = 2, 49, 51, 128, 256
    assert ops.conv_ks_s2_dual_ok(B, H, W, Cin, Cout)
    x = _rand(gen, B, H, W, Cin)
    w = ops.pack_conv_weight_ks_s2_dual(_weight(gen, Cout, Cin, 3), _weight(gen, Cout, Cin, 1))
    sc, sh = _bn(gen, 2 * Cout)
    return (x, lambda: ops.conv2d_ks_s2_dual_nhwc(x, w, sc, sh),
            lambda y, y2: L.lss_conv2d_ks_s2_dual_fwd(p(x), p(w.data), p(sc), p(sh), p(y), p(y2), B, H, W, Cin, Cout, 1,
                                                      ops.N.stream()))


def _k5(ops, gen):
    """The smallest shape the stem plan takes: one 12 x 16 tile per image, 32 workgroups."""
    L, p = ops.N.lib(), ops.N.ptr
    B, H, W = 32, 23, 31
    assert ops.conv_ks_stem_ok(B, H, W, 64, 64)
    x = _rand(gen, B, H, W, 64)
    w = ops.pack_conv_weight_ks_stem(_weight(gen, 64, 64, 7))
    sc, sh = _bn(gen, 64)
    return (x, lambda: ops.conv2d_ks_stem_nhwc(x, w, sc, sh),
            lambda y: L.lss_conv2d_ks_stem_fwd(p(x), p(w.data), p(sc), p(sh), p(y), B, H, W, 64, 64, 1, ops.N.stream()))


CASES = {
    "k0_3x3_c64": (0, lambda o, g: _k0_plain(o, g, 64)),
    "k0_3x3_c128": (0, lambda o, g: _k0_plain(o, g, 128)),
    "k0_fused_up2": (0, _k0_fused_up2),
    "k0_1x1_gelu_f32": (0, _k0_1x1_gelu_f32),
    "k0_fp32": (0, _k0_fp32),
    "k0_ks": (0, _k0_ks),
    "k0_ring": (0, _k0_ring),
    "k1_k1": (1, lambda o, g: _k1(o, g, 1)),
    "k1_k3": (1, lambda o, g: _k1(o, g, 3)),
    "k1_k7": (1, lambda o, g: _k1(o, g, 7)),
    "k2_c128_up2": (2, lambda o, g: _k2(o, g, 1, 8, 8, 64, 128, 2, 4)),
    "k2_c64": (2, lambda o, g: _k2(o, g, 1, 16, 16, 64, 64, 1, 4)),
    "k2_ring": (2, _k2_ring),
    "k3_dual": (3, _k3),
    "k4_ks_s2_dual": (4, _k4),
    "k5_ks_stem": (5, _k5),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_eager_replay_and_abi_entry_agree(ops, name):
    kind, make = CASES[name]
    x, wrapper, entry = make(ops, torch.Generator().manual_seed(sorted(CASES).index(name)))
    as_tuple = lambda r: r if isinstance(r, tuple) else (r,)  # noqa: E731
    eager = [t.clone() for t in as_tuple(wrapper())]
    assert all(bool(t.float().abs().max() > 0) for t in eager), "an all-zero output compares nothing"

    rec = ops.ConvRecorder()
    ops.set_recorder(rec)
    try:
        recorded = as_tuple(wrapper())
    finally:
        ops.set_recorder(None)
    assert [k for k, _ in rec.launches] == [kind]
    plan = ops.ConvPlan(rec, x, recorded[0])
    for t, e in zip(recorded, eager):
        assert torch.equal(t, e)            # the recording pass is an eager pass
        t.fill_(-3.0)
    plan.run(x, recorded[0])
    for t, e in zip(recorded, eager):
        assert torch.equal(t, e), "replayed plan differs from the eager call"
    moved = torch.full_like(recorded[0], -3.0)   # the plan follows its output to another tensor
    plan.run(x, moved)
    assert torch.equal(moved, eager[0])

    outs = [torch.full_like(e, -3.0) for e in eager]
    assert entry(*outs) == 0
    for t, e in zip(outs, eager):
        assert torch.equal(t, e), "the positional ABI entry differs from the eager call"
    ops.assert_no_timeouts("test_conv_launch_gpu " + name)


def test_a_cpu_tensor_in_a_pointer_field_is_refused(ops):
    x = torch.zeros(1, 16, 16, 64, device="cuda").bfloat16()
    w = torch.zeros(9, 64, 64, device="cuda").bfloat16()
    with pytest.raises(ops.N.LssNativeError):
        ops.conv2d_nhwc(x, w, (3, 3), 1, 1, residual=torch.zeros(1, 16, 16, 64).bfloat16())
