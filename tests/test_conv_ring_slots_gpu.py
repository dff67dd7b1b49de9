"""The slot accounting of the ring kernel (csrc/conv_ring.hip): a weight slot is one tap row of three slabs on the plain
and the shared-tile fused instantiations, one slab on the per-strip fused ones.  The smallest shapes at which the slot
hand-off can go wrong (each about 100 workgroups, just over the kernel's floor of 96), per element against the fp64
reference on the bf16-rounded operands and inside the derived bounds of tests/conv_fwd_ref.py - nothing is taken from a
kernel.  Every case runs twice: the runs must agree bit for bit and no flag wait may hit its bound.

The operands follow conv_fwd_ref.make_inputs for a bound case (bf16-valued randn, the per-channel offset + 0.25 randn
source of the fused upsample, scale in [0.5, 1.5], shift ~ 0.1 randn); inputs and references are made once and shared."""
import functools

import pytest
import torch

import conv_fwd_ref as R

pytestmark = pytest.mark.gpu

from lss2_multimodal_nu_amd import ops  # noqa: E402

# name, (B, H, W, Cx, Cout, C2, up, head_n), relu
SLOT_CASES = [
    # one chunk = exactly three slots: the ring never wraps and the last slot is never released to anybody
    ("one_chunk_three_slots", (4, 40, 100, 32, 256, 0, 1, 0), True),
    # six slots: the first refill of every slot (generation 2)
    ("two_chunks_first_refill", (4, 40, 100, 64, 256, 0, 1, 0), False),
    # seven chunks: generations up to 7, an odd chunk count against the two patch buffers
    ("seven_chunks", (4, 40, 100, 224, 256, 0, 1, 0), True),
    # 225 strips: a last workgroup with one live strip of four, ragged columns
    ("ragged_last_workgroup", (5, 36, 90, 64, 256, 0, 1, 0), True),
    # shared-tile fused upsample: 40 x 80 output = whole 8 x 40 tiles, the 7 x 23 source window exactly met
    ("t22_window_met", (5, 20, 40, 64, 256, 0, 2, 0), True),
    # the same with the fused head
    ("t22_head", (10, 20, 40, 64, 128, 0, 2, 4), True),
    # per-strip fused gather, one full-resolution chunk + two upsampled: the instantiation that keeps one-slab slots
    ("strip_fused_one_slab_slots", (4, 10, 25, 64, 256, 32, 4, 0), True),
    # plain conv with the head (also in tests/test_conv_ring_gpu.py; its instantiation takes three-slab slots)
    ("plain_head_n3", (4, 91, 113, 64, 128, 0, 1, 3), True),
]
_BY_NAME = {n: (s, r) for n, s, r in SLOT_CASES}


def _case(name):
    (B, H, W, Cx, Cout, C2, up, head_n), relu = _BY_NAME[name]
    return R._c("slots_" + name, "ring", "ring", "head" if head_n else "s1", "bound", B, H, W, Cx, Cout, C2=C2, up=up,
                relu=relu, head_n=head_n, wpack="ring")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """conv_fwd_ref.make_inputs' recipe for a bound case of the ring kernel.  Shared, never written to."""
    c = _case(name)
    g = R._gen(c.name)
    Cin = c.Cx + c.C2
    if c.up > 1:
        off = (1.0 + 2.0 * torch.rand(1, 1, 1, c.Cx, generator=g)) * (2.0 * torch.randint(0, 2, (1, 1, 1, c.Cx), generator=g) - 1.0)
        x = off + 0.25 * torch.randn(c.B, c.H, c.W, c.Cx, generator=g)
    else:
        x = torch.randn(c.B, c.H, c.W, c.Cx, generator=g)
    x2 = torch.randn(c.B, c.H * c.up, c.W * c.up, c.C2, generator=g) if c.C2 else None
    w = (torch.randn(c.Cout, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5).bfloat16().float()
    scale, shift = torch.rand(c.Cout, generator=g) + 0.5, 0.1 * torch.randn(c.Cout, generator=g)
    head_w = head_b = None
    if c.head_n:
        head_w, head_b = torch.randn(c.head_n, c.Cout, generator=g) * c.Cout ** -0.5, torch.randn(c.head_n, generator=g)
    cast = lambda t: None if t is None else t.bfloat16().contiguous()  # noqa: E731
    return dict(x=cast(x), x2=cast(x2), residual=None, w=w.contiguous(), scale=scale, shift=shift, head_w=head_w,
                head_b=head_b, stats0=None)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return R.ref_conv(_case(name), _inputs(name))


def _run(c, dev):
    if c.head_n:
        return ops.conv3x3_head_nchw(dev["x"], dev["wp"], dev["scale"], dev["shift"], dev["head_w"], dev["head_b"],
                                     x2=dev["x2"], up=c.up, relu=c.relu)
    return ops.conv2d_nhwc(dev["x"], dev["wp"], (3, 3), 1, 1, dev["scale"], dev["shift"], None, c.relu, dev["x2"],
                           c.up, None, 1)


@pytest.mark.parametrize("name", [n for n, _, _ in SLOT_CASES])
def test_slot_case_against_fp64(name, report, monkeypatch):
    monkeypatch.delenv("LSS_CONV_RING", raising=False)
    c = _case(name)
    assert ops.conv_ring_ok(c.B, c.H, c.W, c.Cx, c.C2, c.up, c.Cout, c.head_n), "test shape must be a ring-kernel case"
    assert R.ring_ok(c)
    # the instantiation the case is meant to reach (MODE, HEAD, shared tile): the dispatch of lss_conv_ring_launch as
    # conv_fwd_ref repeats it (its names carry the ring depth of the one-slab form, 7 / 8; the third number is not the point)
    want = {"t22_window_met": "ring<1,0,7,1>", "t22_head": "ring<1,1,7,1>", "strip_fused_one_slab_slots": "ring<1,0,7,0>",
            "plain_head_n3": "ring<0,1,8,0>"}.get(name, "ring<0,0,8,0>")
    assert R.ring_inst(c) == want
    ref = _reference(name)
    assert ref.share <= R.AMBIGUOUS_CAP
    dev = {k: (None if v is None else v.cuda()) for k, v in _inputs(name).items()}
    dev["wp"] = ops.pack_conv_weight_ring(dev["w"])
    before = ops.N.lib().lss_conv2d_ring_timeouts()
    y = _run(c, dev)
    y2 = _run(c, dev)
    assert y.dtype == (torch.float32 if c.head_n else torch.bfloat16)
    y, y2 = y.cpu(), y2.cpu()
    assert ops.N.lib().lss_conv2d_ring_timeouts() == before, "a flag wait of the ring kernel hit its bound"
    assert torch.equal(y, y2), "two runs of the same launch differ"
    tag = "conv_ring_slots." + name
    emax, el2 = R.check(y, ref.out, ref.bound, tag)
    report(tag + ".max", emax)
    report(tag + ".l2", el2)
    report(tag + ".bound_over_max", float(ref.bound.max() / ref.out.abs().max()))
