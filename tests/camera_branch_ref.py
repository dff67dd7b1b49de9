"""fp64 references, DERIVED error bounds, cases and planted errors for the tests of K13, the camera branch of the vovnet
model at inference (tests/test_camera_branch_gpu.py on the GPU, tests/test_camera_branch_ref_cpu.py for this helper):

  lss_tapconv_fwd           ops.tapconv           ref_tapconv      one launch: up to four conv branches, slices, means
  lss_camera_pool_bias_fwd  ops.camera_pool_bias  ref_pool_bias    the ASPP pooling branch as a per-image bias
  VoVNetBEVTransformer.scene_tokens               ref_tokens       c3 -> tokens, composed (with or without rounding)

Rounding points.  Each stage reference computes in fp64 from exactly the operands the kernel multiplies: the bf16
activations it was given and the bf16 weight image (`bf16()` below = round to nearest even, what lss_f2bf does).
Products of bf16 values are exact in fp32; accumulation is fp32; scale, shift, the per-image bias and the ReLU are fp32;
a stored map is rounded to bf16 ONCE; a mean is taken in fp32 over the values as stored.

Bounds (u = 2^-24, the unit roundoff of fp32; none is measured).
  dot product  any fp32 evaluation of a K-term dot product - any order, with or without FMA - satisfies
               |got - ref| <= (K + 2) u S with S = sum |x w|, K = live taps x Cin (Higham's gamma_K S, K u < 0.01 here).
               The per-image bias is one more term: S gains |bias|, K gains 1.
  epilogue     v = max(scale (a + bias) + shift, 0), with or without FMA; the ReLU is 1-Lipschitz:
                   E_v = |scale| E_a + 2 u (|scale (a + bias)| + |shift|).
  bf16 store   one round-to-nearest-even of a value t within E_v of v moves it by at most half a bf16 ulp of t,
               2^-9 of the binade's upper end 2^(floor(log2 t) + 1):  E_y = E_v + half_ulp_bf16(|v| + E_v).  (Relative
               to |t| itself that is between 2^-9 and 2^-8: 1.00393895 lies 2^-8 from both of its bf16 neighbours 1.0
               and 1.0078125, so "2^-9 |t|" is not attainable by any correctly rounding store; half an ulp is the
               format's own figure and is what is asserted.)
  mean         HW - 1 additions and one division in fp32, any order: (HW + 1) u mean|y| on top of the mean of the
               elementwise bounds of what is averaged.
  pool bias    g and bias are dot products of fp32 operands: (K + 2) u S each, the second carrying |wj| E_g.

`check(got, ref, bound)` is depth_head_ref's.  A reference called with `plant=` returns, in its `*_sim` fields, what a
kernel with that defect would write; every plant moves an output by a whole product, a whole pixel or a whole bf16 ulp,
and the CPU test proves `check` rejects each.  A case that cannot show a plant raises `NotExercised`.
"""
import collections

import torch

from depth_head_ref import U32, NotExercised, check  # noqa: F401  (re-exported)
from train_node_ref import errors  # noqa: F401  (re-exported)



def half_ulp_bf16(t):
    """Half a bf16 ulp (8 significant bits) at magnitude t >= 0: 2^(floor(log2 t) - 8); 0 at 0."""
    _, e = torch.frexp(t.double())          # t = m 2^e, m in [0.5, 1)
    return torch.where(t > 0, torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 9), torch.zeros_like(t, dtype=torch.float64))


TILE = 64  # pixel rows per tile of tapconv_kernel: what a partial tile is partial of
PLANTS = ("tap_from_neighbour_image", "dead_tap_clamped", "dilations_swapped", "slice_offset_wrong",
          "pool_counts_padding_rows", "mean_divides_by_tile_rows", "image_bias_dropped", "bf16_truncated")

# (name, BN, Cin, H, W): the shapes of the issue's table; the sixth (slice) case is SLICE below
Case = collections.namedtuple("Case", "name BN Cin H W")
CASES = [
    Case("production", 6, 768, 8, 22),     # twelve Cin blocks; 3 / 1 / 1 live ASPP taps
    Case("hires", 2, 128, 16, 44),         # r = 12 with all nine taps half-live; r = 24 and 36 with three
    Case("partial_3x5", 3, 64, 3, 5),      # 15 pixels in a partial tile; d = 2 alive in rows 0 and 2 only
    Case("strip_2x13", 2, 64, 2, 13),      # r = 12 alive in one column each side
    Case("pixel_1x1", 2, 64, 1, 1),        # every off-centre tap dead, even d = 1; mean of one pixel
]
SLICE = Case("slice_5x7", 1, 128, 5, 7)    # Cout 64 into channels 64..127 of a 192-wide buffer
MID = 256
PYRAMID_DILATIONS = (1, 2)
ASPP_RATES = (12, 24, 36)


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def bf16(t):
    """Round to nearest even to bf16, kept as fp32 values."""
    return t.float().bfloat16().float()


def bf16_trunc(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def live_taps(H, W, ksize, dilation):
    """Taps ky * 3 + kx that can reach an (H, W) map; written from the definition, not from the product's list."""
    if ksize == 1:
        return [0]
    out = []
    for ky in (-1, 0, 1):
        for kx in (-1, 0, 1):
            if abs(ky * dilation) < H and abs(kx * dilation) < W:
                out.append((ky + 1) * 3 + (kx + 1))
    return out


def aspp_live_count(H, W, rates=ASPP_RATES):
    return sum(len(live_taps(H, W, 3, r)) for r in rates)


# ----------------------------------------------------------------------------------------------------------------------
# one launch
# ----------------------------------------------------------------------------------------------------------------------
Branch = collections.namedtuple("Branch", "w dilation scale shift ch_off")  # w (Cout, Cin, k, k) holding bf16 values
Stage = collections.namedtuple("Stage", "y bound_y mean bound_mean y_sim mean_sim")


def make_branch(name, Cout, Cin, ksize, dilation, ch_off, bias_like_shift=True):
    g = _gen(name)
    w = bf16(torch.randn(Cout, Cin, ksize, ksize, generator=g) / (Cin * ksize * ksize) ** 0.5)
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = 0.3 * torch.randn(Cout, generator=g) + 0.1   # relu(shift) != 0 on most channels: padding rows show
    return Branch(w, dilation, scale, shift, ch_off)


def make_input(name, BN, H, W, C):
    return bf16(torch.randn(BN, H, W, C, generator=_gen(name + ".x")))


def _shifted(x, dy, dx, plant):
    """x (BN, H, W, C) fp64 read at (h + dy, w + dx): zero outside the map (the contract)."""
    BN, H, W, C = x.shape
    if plant == "dead_tap_clamped":
        hi = (torch.arange(H) + dy).clamp(0, H - 1)
        wi = (torch.arange(W) + dx).clamp(0, W - 1)
        return x[:, hi][:, :, wi]
    src = x
    if plant == "tap_from_neighbour_image":  # rows are taken from the flat (BN * H) row index: no image boundary
        src = x.reshape(1, BN * H, W, C)
    n, R = src.shape[0], src.shape[1]
    out = torch.zeros_like(src)
    h0, h1 = max(0, -dy), min(R, R - dy)
    w0, w1 = max(0, -dx), min(W, W - dx)
    if h0 < h1 and w0 < w1:
        out[:, h0:h1, w0:w1] = src[:, h0 + dy:h1 + dy, w0 + dx:w1 + dx]
    return out.reshape(BN, H, W, C)


def ref_tapconv(x, branches, y_width=None, img_bias=None, relu=True, store=True, want_mean=False, plant=None):
    """x (BN, H, W, Cin) holding bf16 values; branches: `Branch`es; y_width: channels of the output buffer (default: the
    branches side by side).  Returns Stage: y / bound_y (BN, H, W, y_width) fp64 - 0 / 0 where no branch writes -, mean /
    bound_mean (BN, Cout) of branch 0 when want_mean, and the simulated kernel outputs (bf16-rounded map as fp32, fp32
    mean), which carry the planted error if any."""
    if plant is not None and plant not in PLANTS:
        raise ValueError(plant)
    BN, H, W, Cin = x.shape
    HW = H * W
    x64 = x.double()
    Cout = branches[0].w.shape[0]
    if y_width is None:
        y_width = max(b.ch_off for b in branches) + Cout
    # channels no branch writes: the buffer is taken as zero-filled and must stay so
    y = torch.zeros(BN, H, W, y_width, dtype=torch.float64)
    by = torch.zeros(BN, H, W, y_width, dtype=torch.float64)
    ysim = torch.zeros(BN, H, W, y_width, dtype=torch.float32)
    mean = bmean = msim = None
    dil = [b.dilation for b in branches]
    if plant == "dilations_swapped":
        three = [i for i, b in enumerate(branches) if b.w.shape[2] == 3]
        pair = [(i, j) for i in three for j in three if i < j and dil[i] != dil[j]
                and (len(live_taps(H, W, 3, dil[i])) > 1 or len(live_taps(H, W, 3, dil[j])) > 1)]
        if not pair:
            raise NotExercised("needs two 3x3 branches whose dilations give different sums")
        i, j = pair[0]
        dil[i], dil[j] = dil[j], dil[i]
    if plant == "tap_from_neighbour_image" and (BN < 2 or not any(
            b.w.shape[2] == 3 and any(t // 3 != 1 for t in live_taps(H, W, 3, b.dilation)) for b in branches)):
        raise NotExercised("needs a second image and a live tap that leaves the map vertically")
    if plant == "dead_tap_clamped" and all(len(live_taps(H, W, b.w.shape[2], b.dilation)) == 1 for b in branches):
        raise NotExercised("only centre taps are live: nothing leaves the map")
    if plant == "image_bias_dropped" and img_bias is None:
        raise NotExercised("no per-image bias")
    if plant in ("pool_counts_padding_rows", "mean_divides_by_tile_rows") and (not want_mean or HW % TILE == 0):
        raise NotExercised("needs a mean over an image whose last tile is partial")
    if plant in ("bf16_truncated", "slice_offset_wrong") and not store:
        raise NotExercised("no map is stored")
    for bi, b in enumerate(branches):
        k = b.w.shape[2]
        w64 = b.w.double()

        def conv(d, shift_plant):
            a = torch.zeros(BN, H, W, Cout, dtype=torch.float64)
            S = torch.zeros_like(a)
            taps = live_taps(H, W, k, d)
            for t in taps:
                ky, kx = (t // 3 - 1, t % 3 - 1) if k == 3 else (0, 0)
                xs = _shifted(x64, ky * d, kx * d, shift_plant)
                wt = w64[:, :, ky + 1, kx + 1] if k == 3 else w64[:, :, 0, 0]
                a += xs @ wt.t()
                S += xs.abs() @ wt.abs().t()
            return a, S, len(taps) * Cin

        def epilogue(a, ib):
            sc, sh = b.scale.double(), b.shift.double()
            pre = (a + ib) * sc
            v = pre + sh
            return (torch.relu(v) if relu else v), pre, sh

        ib = torch.zeros(BN, 1, 1, Cout, dtype=torch.float64) if img_bias is None else img_bias.double().view(BN, 1, 1, Cout)
        a, S, K = conv(b.dilation, None)
        v, pre, sh = epilogue(a, ib)
        E_a = (K + 2 + (img_bias is not None)) * U32 * (S + ib.abs())
        E_v = b.scale.double().abs() * E_a + 2 * U32 * (pre.abs() + sh.abs())
        E_y = E_v + half_ulp_bf16(v.abs() + E_v) if store else E_v
        # what the (possibly defective) kernel computes
        pa, _, _ = conv(dil[bi], plant if plant in ("tap_from_neighbour_image", "dead_tap_clamped") else None)
        pv, _, _ = epilogue(pa, torch.zeros_like(ib) if plant == "image_bias_dropped" else ib)
        if store:
            stored = bf16_trunc(pv) if plant == "bf16_truncated" else bf16(pv)
            off = b.ch_off + (4 if plant == "slice_offset_wrong" else 0)
            if off + Cout > y_width:
                off = b.ch_off - 4
                if off < 0:
                    raise NotExercised("the buffer has no room to misplace the slice")
            ysim[..., off:off + Cout] = stored
            y[..., b.ch_off:b.ch_off + Cout] = v
            by[..., b.ch_off:b.ch_off + Cout] = E_y
        else:
            stored = pv.float()
        if want_mean and bi == 0:
            mean = v.reshape(BN, HW, Cout).mean(1)
            bmean = E_y.reshape(BN, HW, Cout).mean(1) + (HW + 1) * U32 * (v.abs() + E_y).reshape(BN, HW, Cout).mean(1)
            tot = stored.double().reshape(BN, HW, Cout).sum(1)
            npad = (-HW) % TILE
            if plant == "pool_counts_padding_rows":   # a padding row holds act(scale * bias + shift), not 0
                padv, _, _ = epilogue(torch.zeros(BN, 1, 1, Cout, dtype=torch.float64), ib)
                padv = padv.reshape(BN, Cout)
                if not bool((padv != 0).any()):
                    raise NotExercised("every padding row is cut to zero")
                tot = tot + npad * padv
            div = HW + npad if plant == "mean_divides_by_tile_rows" else HW
            msim = (tot / div).float()
    return Stage(y, by, mean, bmean, ysim, msim)


PoolBias = collections.namedtuple("PoolBias", "g bound_g bias bound_bias")


def ref_pool_bias(mean, wg, scale, shift, wj):
    """mean (BN, C), wg (Cg, C), scale / shift (Cg), wj (Cout, Cg), all fp32 values -> g (BN, Cg), bias (BN, Cout)."""
    m, wg64, wj64 = mean.double(), wg.double(), wj.double()
    C, Cg = wg.shape[1], wg.shape[0]
    a, S = m @ wg64.t(), m.abs() @ wg64.abs().t()
    pre = a * scale.double()
    g = torch.relu(pre + shift.double())
    E_g = scale.double().abs() * (C + 2) * U32 * S + 2 * U32 * (pre.abs() + shift.double().abs())
    bias = g @ wj64.t()
    E_b = (Cg + 2) * U32 * ((g + E_g) @ wj64.abs().t()) + E_g @ wj64.abs().t()
    return PoolBias(g, E_g, bias, E_b)


# ----------------------------------------------------------------------------------------------------------------------
# composed: c3 -> tokens from the two modules' parameters
# ----------------------------------------------------------------------------------------------------------------------
def fold(conv, bn):
    """(w OIHW, scale, shift) in fp64, as `_FoldedConv.get` folds them (the conv bias goes into the shift)."""
    inv = torch.rsqrt(bn.running_var.double() + bn.eps)
    scale = bn.weight.double() * inv
    mean = bn.running_mean.double()
    if conv.bias is not None:
        mean = mean - conv.bias.double()
    return conv.weight.detach().double(), scale.detach(), (bn.bias.double() - mean * scale).detach()


def ref_tokens(c3, pyramid, sceneunder, rounding=True):
    """The contract of K13 in fp64: live taps only, the pooled branch as a per-image bias, the mean of the projection.
    rounding=True rounds x, the conv weights and the stored y_b, p, a_i to bf16 (the bf16 route's rounding points);
    rounding=False rounds nothing: then this IS the module composition, restated.  c3 (BN, Cin, H, W), on the modules'
    device (only gathers and fp64 matrix products: it runs wherever they are).  Returns (tokens (BN, 256), mean_p
    (BN, 256)) fp64."""
    r = (lambda t: bf16(t).double()) if rounding else (lambda t: t.double())
    aspp = sceneunder[0]
    x = r(c3.permute(0, 2, 3, 1))
    BN, H, W, _ = x.shape

    def run(xin, conv, bn, img_bias=None, wcols=None):
        w, sc, sh = fold(conv, bn)
        if wcols is not None:
            w = w[:, wcols]
        k, d = conv.kernel_size[0], conv.dilation[0]
        a = torch.zeros(BN, H, W, w.shape[0], dtype=torch.float64, device=xin.device)
        for t in live_taps(H, W, k, d):
            ky, kx = (t // 3 - 1, t % 3 - 1) if k == 3 else (0, 0)
            wt = r(w[:, :, ky + 1, kx + 1] if k == 3 else w[:, :, 0, 0])
            a += _shifted(xin, ky * d, kx * d, None) @ wt.t()
        if img_bias is not None:
            a = a + img_bias.view(BN, 1, 1, -1)
        return torch.relu(a * sc + sh)

    ys = [r(run(x, b[0], b[1])) for b in (pyramid.scale1, pyramid.scale2)]
    p = r(run(torch.cat(ys, 3), pyramid.fusion[0], pyramid.fusion[1]))
    mean_p = p.mean((1, 2))
    convs = list(aspp.convs)
    cat = torch.cat([r(run(p, c[0], c[1])) for c in convs[:4]], 3)
    wg, gsc, gsh = fold(convs[4][1], convs[4][2])
    g = torch.relu((mean_p @ wg[:, :, 0, 0].t()) * gsc + gsh)
    wj = aspp.project[0].weight.detach().double()[:, :, 0, 0]
    n = cat.shape[3]
    s = run(cat, aspp.project[0], aspp.project[1], img_bias=g @ wj[:, n:].t(), wcols=slice(0, n))
    return s.mean((1, 2)), mean_p


def state_shapes(module):
    """Ordered (key, shape) pairs of a module's state_dict: the shape list `oracle.vovnet_oracle.seeded_state` takes."""
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
