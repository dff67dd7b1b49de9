"""fp64 references, DERIVED error bounds, cases and planted errors for the tests of K15, the TXT half of BEV_TXT at
inference behind the ASPP (tests/test_txt_heads_gpu.py on the GPU, tests/test_txt_heads_ref_cpu.py for this helper):

  lss_bev_post_fwd   ops.bev_post   ref_bev_post    crop -> conv 3x3 / (2, 1) / pad 1 -> scale, shift, ReLU -> MaxPool (5, 4)
  lss_txt_heads_fwd  ops.txt_heads  ref_txt_heads   embedder conv, concat, Linear, predictors

Rounding points.  Each reference computes in fp64 from exactly the operands the kernel multiplies: the bf16 scene map
and the bf16 embedder weight image (`bf16()` = round to nearest even), fp32 everything else.  Products of bf16 values
are exact in fp32, accumulation is fp32; the embedder output is NOT rounded to bf16.

Bounds (u = 2^-24, the unit roundoff of fp32; none is measured).
  dot product  any fp32 evaluation of a K-term dot product - any order, with or without FMA - satisfies
               |got - ref| <= (K + 2) u S, S = sum |x w| (Higham's gamma_K S, K u < 0.01 here).  K = live taps x 256 for
               the embedder conv, 9 Cb for BevPost, (32 + Cp) HW + 1 for the Linear (the bias is one more term, and S
               gains |bias|), E + 1 for a predictor.
  epilogue     v = max(scale a + shift, 0), with or without FMA; the ReLU is 1-Lipschitz (K13's rule):
                   E_v = |scale| E_a + 2 u (|scale a| + |shift|).
  max pool     the maximum is 1-Lipschitz in the sup norm: the bound of a pooled value is the largest bound in its window.
  carried      an operand that is itself within E of its reference enters the next product through |W|:
                   E_y = (K + 2) u (|W| (|V| + E_V) + |b|) + |W| E_V,      the same for a predictor over y.

`check(got, ref, bound)` is depth_head_ref's.  A reference called with `plant=` returns, in its `*_sim` fields, what a
kernel with that defect would write; every plant moves an output by a whole product or a whole pixel, and the CPU test
proves `check` rejects each.  A case that cannot show a plant raises `NotExercised`.  `embed_rounded_to_bf16` moves every
embedder value by up to half a bf16 ulp of either sign, which averages out over the hundreds of values a Linear row
adds: it shows where few are added (pixel_1x1), and only there is it required to be rejected.
"""
import collections

import torch

from camera_branch_ref import _shifted, bf16, live_taps
from depth_head_ref import U32, NotExercised, check  # noqa: F401  (re-exported)
from train_node_ref import errors  # noqa: F401  (re-exported)

TILE = 16   # pixels per tile of txt_heads_tile_kernel: what a partial tile is partial of
EMBED = 32  # embedder channels
SCENE = 256
PROD_CAMS = (1, 0, 3, 2, 5)
POST_PLANTS = ("conv_reads_outside_crop", "stride_transposed", "pool_window_transposed", "crop_origin_swapped")
HEAD_PLANTS = ("tap_from_neighbour_image", "padding_rows_enter_linear", "flatten_pixel_major", "bev_post_before_embed",
               "side_cameras_in_index_order", "front_predictors_swapped", "side_uses_front_weights",
               "embed_rounded_to_bf16")
PLANTS = HEAD_PLANTS + POST_PLANTS

# name, B, H x W of the scene map, BEV map size, crop origin, crop size, Cb, Cp, ncams, slot table, E, n_act, n_desc_f
Case = collections.namedtuple("Case", "name B H W map origin crop Cb Cp ncams cams E n_act n_desc_f")
CASES = [
    Case("production", 2, 8, 22, (200, 200), (60, 56), (80, 88), 4, 8, 6, PROD_CAMS, 40, 4, 4),  # 11 full tiles
    Case("partial_3x5", 3, 3, 5, (40, 30), (5, 7), (30, 20), 3, 5, 6, PROD_CAMS, 40, 4, 4),       # one partial tile
    Case("tiles_5x7", 2, 5, 7, (50, 28), (0, 0), (50, 28), 8, 8, 6, PROD_CAMS, 64, 4, 4),         # 2 tiles + 3 rows
    Case("pixel_1x1", 2, 1, 1, (12, 6), (1, 1), (10, 4), 1, 1, 6, PROD_CAMS, 7, 3, 5),            # centre tap only
    Case("one_slot", 1, 3, 5, (40, 30), (5, 7), (30, 20), 4, 8, 2, (1,), 40, 4, 4),               # front slot only
]
BY_NAME = {c.name: c for c in CASES}
# the crop of tiles_5x7 IS the map, so Hc - 1 is odd there; the even one (Hc = 49) gives the same 5 x 7 output
POST_EXTRA = [BY_NAME["tiles_5x7"]._replace(name="tiles_5x7_h49", crop=(49, 28))]


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def post_out_size(Hc, Wc):
    return (((Hc - 1) // 2) + 1) // 5, Wc // 4


# ----------------------------------------------------------------------------------------------------------------------
# BevPost
# ----------------------------------------------------------------------------------------------------------------------
Post = collections.namedtuple("Post", "y bound y_sim")


def make_post_inputs(c):
    """(map (B, Cb, Hm, Wm), w (Cp, Cb, 3, 3), scale (Cp), shift (Cp)) fp32."""
    g = _gen(c.name + ".post")
    m = torch.randn(c.B, c.Cb, *c.map, generator=g)
    w = torch.randn(c.Cp, c.Cb, 3, 3, generator=g) / (9 * c.Cb) ** 0.5
    return m, w, torch.rand(c.Cp, generator=g) + 0.5, 0.3 * torch.randn(c.Cp, generator=g) + 0.1


def _post_eval(m64, origin, crop, w64, scale, shift, Cb, outside_zero=True, stride=(2, 1), window=(5, 4)):
    """(pooled (B, Co, Ho, Wo), pooled bound) in fp64, from the definition: a gather per tap, no library conv / pool."""
    (h0, w0), (Hc, Wc) = origin, crop
    B, _, Hm, Wm = m64.shape
    Hconv, Wconv = (Hc - 1) // 2 + 1, Wc
    Ho, Wo = post_out_size(Hc, Wc)

    def read(rows, cols):
        """The crop at (rows x cols) in crop coordinates; zero outside the crop (the contract) - or, planted, whatever
        the map holds there, and zero outside the map."""
        if outside_zero:
            okr, okc = (rows >= 0) & (rows < Hc), (cols >= 0) & (cols < Wc)
        else:
            okr, okc = (rows + h0 >= 0) & (rows + h0 < Hm), (cols + w0 >= 0) & (cols + w0 < Wm)
        rr, cc = (rows + h0).clamp(0, Hm - 1), (cols + w0).clamp(0, Wm - 1)
        v = m64[:, :, rr][:, :, :, cc]
        return v * (okr[:, None] & okc[None, :]).double()

    r, cidx = torch.arange(Hconv), torch.arange(Wconv)
    a = torch.zeros(B, w64.shape[0], Hconv, Wconv, dtype=torch.float64)
    S = torch.zeros_like(a)
    for ky in range(3):
        for kx in range(3):
            v = read(stride[0] * r - 1 + ky, stride[1] * cidx - 1 + kx)
            a += torch.einsum("bchw,oc->bohw", v, w64[:, :, ky, kx])
            S += torch.einsum("bchw,oc->bohw", v.abs(), w64[:, :, ky, kx].abs())
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    pre = a * sc
    v = torch.relu(pre + sh)
    E_v = sc.abs() * (9 * Cb + 2) * U32 * S + 2 * U32 * (pre.abs() + sh.abs())
    y = torch.zeros(B, w64.shape[0], Ho, Wo, dtype=torch.float64)
    E = torch.zeros_like(y)
    for i in range(Ho):
        for j in range(Wo):
            r0, c0 = window[0] * i, window[1] * j
            win = (slice(None), slice(None), slice(r0, min(r0 + window[0], Hconv)), slice(c0, min(c0 + window[1], Wconv)))
            if v[win].numel() == 0:
                continue
            y[:, :, i, j] = v[win].amax((2, 3))
            E[:, :, i, j] = E_v[win].amax((2, 3))
    return y, E


def ref_bev_post(m, origin, crop, w, scale, shift, plant=None):
    """m (B, Cb, Hm, Wm) fp32 -> Post(y, bound, y_sim): the contract in fp64, its derived bound, and what a kernel (with
    the planted defect, if any) would write."""
    if plant is not None and plant not in POST_PLANTS:
        raise ValueError(plant)
    m64, w64, Cb = m.double(), w.double(), m.shape[1]
    (h0, w0), (Hc, Wc) = origin, crop
    Hm, Wm = m.shape[2:]
    y, E = _post_eval(m64, origin, crop, w64, scale, shift, Cb)
    kw = {}
    o = origin
    if plant == "conv_reads_outside_crop":
        if h0 == 0 and w0 == 0 and h0 + Hc == Hm and w0 + Wc == Wm:
            raise NotExercised("the crop is the map: nothing lies beyond it")
        kw["outside_zero"] = False
    elif plant == "stride_transposed":
        kw["stride"] = (1, 2)
    elif plant == "pool_window_transposed":
        kw["window"] = (4, 5)
    elif plant == "crop_origin_swapped":
        if h0 == w0 or w0 + Hc > Hm or h0 + Wc > Wm:
            raise NotExercised("the swapped origin is the same crop or leaves the map")
        o = (w0, h0)
    sim, _ = _post_eval(m64, o, crop, w64, scale, shift, Cb, **kw)
    return Post(y, E, sim.float())


# ----------------------------------------------------------------------------------------------------------------------
# the heads
# ----------------------------------------------------------------------------------------------------------------------
HeadSet = collections.namedtuple("HeadSet", "w scale shift lin_w lin_b")  # w (32, 256, 3, 3) holding bf16 values
Heads = collections.namedtuple("Heads", "act bound_act desc bound_desc act_sim desc_sim")


def make_head_inputs(c):
    """(scene (B ncams, H, W, 256) bf16 values, bev_post (B, Cp, H, W), front, side, predictors), all fp32 tensors."""
    g = _gen(c.name + ".heads")
    HW = c.H * c.W
    # every camera at its own level (x 0.5, 0.75, 1, ...): a slot that reads the wrong camera is off by a whole factor
    level = 0.5 + 0.25 * (torch.arange(c.B * c.ncams) % c.ncams).float().view(-1, 1, 1, 1)
    scene = bf16(torch.relu(torch.randn(c.B * c.ncams, c.H, c.W, SCENE, generator=g)) * level)
    post = torch.relu(torch.randn(c.B, c.Cp, c.H, c.W, generator=g))
    K = (EMBED + c.Cp) * HW

    # Weights with a positive mean over non-negative activations: the sums do not cancel, S = sum |x w| stays close to
    # |sum x w|, and the (K + 2) u S bounds are a few 1e-4 of the values themselves instead of a multiple of them
    def one_set():
        w = bf16((0.5 * torch.randn(EMBED, SCENE, 3, 3, generator=g) + 1.0) / (9 * SCENE))
        scale = torch.rand(EMBED, generator=g) + 0.5
        shift = 0.3 * torch.randn(EMBED, generator=g) + 0.1  # relu(shift) != 0 on most channels: padding rows show
        return HeadSet(w, scale, shift, (0.5 * torch.randn(c.E, K, generator=g) + 1.0) / K,
                       0.1 * torch.randn(c.E, generator=g))

    front, side = one_set(), one_set()
    pred = {}
    for k, n in (("f1", c.n_desc_f), ("f2", c.n_act), ("lr", 1)):
        pred[k + "_w"] = (0.5 * torch.randn(n, c.E, generator=g) + 1.0) / c.E
        pred[k + "_b"] = 0.1 * torch.randn(n, generator=g)
    return scene, post, front, side, pred


def _embed(x64, hs, plant):
    """(e, E_e) (BN, H, W, 32) fp64: relu(scale conv + shift) over every image, and its bound."""
    BN, H, W, _ = x64.shape
    w64 = hs.w.double()
    a = torch.zeros(BN, H, W, EMBED, dtype=torch.float64)
    S = torch.zeros_like(a)
    taps = live_taps(H, W, 3, 1)
    for t in taps:
        ky, kx = t // 3 - 1, t % 3 - 1
        xs = _shifted(x64, ky, kx, plant if plant == "tap_from_neighbour_image" else None)
        a += xs @ w64[:, :, ky + 1, kx + 1].t()
        S += xs.abs() @ w64[:, :, ky + 1, kx + 1].abs().t()
    sc, sh = hs.scale.double(), hs.shift.double()
    pre = a * sc
    e = torch.relu(pre + sh)
    E_e = sc.abs() * (len(taps) * SCENE + 2) * U32 * S + 2 * U32 * (pre.abs() + sh.abs())
    if plant == "embed_rounded_to_bf16":
        e = bf16(e).double()
    return e, E_e


def _affine(w, b, v, E_v):
    """(y, E_y) of y = b + w v over the last axis of v, with the carried bound."""
    w64, b64 = w.double(), b.double()
    K = w.shape[1] + 1
    y = v @ w64.t() + b64
    E_y = (K + 2) * U32 * ((v.abs() + E_v) @ w64.abs().t() + b64.abs()) + E_v @ w64.abs().t()
    return y, E_y


def ref_txt_heads(scene, post, front, side, pred, cams, ncams, plant=None):
    """The contract of lss_txt_heads_fwd in fp64 -> Heads(act, bound_act, desc, bound_desc, act_sim, desc_sim)."""
    if plant is not None and plant not in HEAD_PLANTS:
        raise ValueError(plant)
    BN, H, W, _ = scene.shape
    B, Cp, HW = BN // ncams, post.shape[1], H * W
    n_slots = len(cams)
    if plant == "tap_from_neighbour_image" and H < 2:
        raise NotExercised("no tap leaves the map vertically")
    if plant == "flatten_pixel_major" and HW == 1:
        raise NotExercised("one pixel: both flatten orders are the same")
    if plant == "padding_rows_enter_linear" and HW % TILE == 0:
        raise NotExercised("every tile is full")
    if plant == "side_uses_front_weights" and n_slots < 2:
        raise NotExercised("no side slot")
    if plant == "side_cameras_in_index_order" and tuple(cams) != PROD_CAMS:
        raise NotExercised("not the production slot table")
    if plant == "front_predictors_swapped" and pred["f1_w"].shape != pred["f2_w"].shape:
        raise NotExercised("the two front predictors differ in size")
    x64, p64 = scene.double(), post.double()

    def run(plant):
        sets = (front, front if plant == "side_uses_front_weights" else side)
        table = (1, 0, 2, 3, 5) if plant == "side_cameras_in_index_order" else cams
        emb = [_embed(x64, s, plant) for s in (sets if n_slots > 1 else sets[:1])]
        ys = []
        for s, cam in enumerate(table):
            hs = sets[0 if s == 0 else 1]
            e, E_e = emb[0 if s == 0 else 1]
            e, E_e = e[cam::ncams], E_e[cam::ncams]                                  # (B, H, W, 32)
            e, E_e = e.permute(0, 3, 1, 2), E_e.permute(0, 3, 1, 2)                  # (B, 32, H, W)
            parts, bounds = [e, p64], [E_e, torch.zeros_like(p64)]
            if plant == "bev_post_before_embed":
                parts, bounds = parts[::-1], bounds[::-1]
            v, E_v = torch.cat(parts, 1), torch.cat(bounds, 1)                        # (B, 32 + Cp, H, W)
            if plant == "flatten_pixel_major":
                v, E_v = v.permute(0, 2, 3, 1), E_v.permute(0, 2, 3, 1)
            v, E_v = v.reshape(B, -1), E_v.reshape(B, -1)
            y, E_y = _affine(hs.lin_w, hs.lin_b, v, E_v)
            if plant == "padding_rows_enter_linear":
                # the rows HW .. of the last tile hold relu(shift) and meet the weight columns that follow theirs
                npad, lw = (-HW) % TILE, hs.lin_w.double()
                padv = torch.relu(hs.shift.double())
                if not bool((padv != 0).any()):
                    raise NotExercised("every padding row is cut to zero")
                for c in range(EMBED):
                    cols = c * HW + HW + torch.arange(npad)
                    cols = cols[cols < lw.shape[1]]
                    y = y + padv[c] * lw[:, cols].sum(1)
            ys.append((y, E_y))
        f1, f2 = ("f2", "f1") if plant == "front_predictors_swapped" else ("f1", "f2")
        desc_f, E_df = _affine(pred[f1 + "_w"], pred[f1 + "_b"], *ys[0])
        act, E_a = _affine(pred[f2 + "_w"], pred[f2 + "_b"], *ys[0])
        sides = [_affine(pred["lr_w"], pred["lr_b"], *ys[s]) for s in range(1, n_slots)]
        desc = torch.cat([desc_f] + [s[0] for s in sides], 1)
        E_d = torch.cat([E_df] + [s[1] for s in sides], 1)
        return act, E_a, desc, E_d

    act, E_a, desc, E_d = run(None)
    sa, _, sd, _ = run(plant)
    return Heads(act, E_a, desc, E_d, sa.float(), sd.float())


def torch_heads(c, scene, post, front, side, pred):
    """The same computation on the project's own modules (heads.py) in fp64: (act, desc).  What ref_txt_heads restates."""
    from lss2_multimodal_nu_amd import heads
    HW = c.H * c.W

    def embedder(cls1, hs):
        e1 = cls1(SCENE, EMBED).double().eval()
        e1[0].weight.data.copy_(hs.w.double())
        # an eval BatchNorm with mean 0, var 1 - eps, weight = scale, bias = shift is exactly (scale, shift)
        e1[1].running_mean.zero_()
        e1[1].running_var.fill_(1.0 - e1[1].eps)
        e1[1].weight.data.copy_(hs.scale.double())
        e1[1].bias.data.copy_(hs.shift.double())
        lin = torch.nn.Linear((EMBED + c.Cp) * HW, c.E).double()
        lin.weight.data.copy_(hs.lin_w.double())
        lin.bias.data.copy_(hs.lin_b.double())
        return e1, torch.nn.Sequential(torch.nn.Flatten(), lin)

    def predictor(k):
        p = heads.Predictor(c.E, pred[k + "_w"].shape[0]).double()
        p[0].weight.data.copy_(pred[k + "_w"].double())
        p[0].bias.data.copy_(pred[k + "_b"].double())
        return p

    f1, f2 = embedder(heads.Embedder_f1, front)
    l1, l2 = embedder(heads.Embedder_lr1, side)
    s64 = scene.double().permute(0, 3, 1, 2)
    p64 = post.double()
    with torch.no_grad():
        y_f = f2(torch.cat([f1(s64[c.cams[0]::c.ncams]), p64], 1))
        desc = [predictor("f1")(y_f)]
        act = predictor("f2")(y_f)
        for cam in c.cams[1:]:
            desc.append(predictor("lr")(l2(torch.cat([l1(s64[cam::c.ncams]), p64], 1))))
    return act, torch.cat(desc, 1)


def torch_bev_post(c, m, w, scale, shift):
    """heads.BevPost in fp64 on the crop: what ref_bev_post restates."""
    from lss2_multimodal_nu_amd import heads
    bp = heads.BevPost(c.Cb, c.Cp).double().eval()
    bp.post[0].weight.data.copy_(w.double())
    bp.post[1].running_mean.zero_()
    bp.post[1].running_var.fill_(1.0 - bp.post[1].eps)
    bp.post[1].weight.data.copy_(scale.double())
    bp.post[1].bias.data.copy_(shift.double())
    (h0, w0), (Hc, Wc) = c.origin, c.crop
    with torch.no_grad():
        return bp(m.double()[:, :, h0:h0 + Hc, w0:w0 + Wc])
