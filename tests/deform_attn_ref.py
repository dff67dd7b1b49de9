"""fp64 references, DERIVED error bounds, cases and planted errors for the tests of the BEV transformer's deformable-
attention core and of add_pos alone (tests/test_deform_attn_fwd_gpu.py on the GPU, tests/test_deform_attn_ref_cpu.py for
this helper itself):

  deform_attn   deform_attn_kernel<T, PTS>   ops.deform_attn / ops.deform_attn_pts   ref_deform_attn
  add_pos       add_pos_kernel<T>            ops.add_pos                             ref_add_pos

Everything is fp64 on the CPU.  u = 2^-24 is the unit roundoff of fp32.  No bound is measured on a kernel.

Operands.  The reference reads what the kernel reads: fp32 offsets_logits, token_bias, ref_x / ref_y or ref_pts, widened
exactly; `value` at its own fp32 or bf16 values.  With a token_bias the kernel first forms fl(ol + bias) in fp32 while the
reference adds in fp64: every offset and logit then enters with an operand error e_in = u |ol + bias| (e_in = 0 without
a bias; `input_err=` adds a caller's own operand perturbation on top, which is how the bias form is compared with the
reference of the undivided problem).

The operation, per (sample, token, head), over its 8 points p and the 32 channels c of the head:
    aw   = softmax_p(logit)
    loc  = clamp(ref + off / H, 0, 1)            BOTH axes are divided by H (the reference model's behaviour)
    px   = loc_x W - 0.5,  py = loc_y H - 0.5
    f_p  = zero-padded bilinear interpolant of value[.., head, c] at (px, py)
    out  = sum_p aw_p f_p

Softmax weight.  As in depth_head_ref: perturbing every logit by at most eps moves a weight by a factor within
exp(+-2 eps).  Here eps = max_p (e_in + u |logit_p - max|): the operand error and the rounding of the subtraction of the
(exactly found) maximum.  expf at 1 ulp (2u), the 8-term sum (7 additions of terms that carry expf's 2u) and the division
(u) add at most (8 + 8) u as there:
    e_aw = aw (expm1(2 eps) + 16 u) + 2^-126           (a weight below the smallest normal number may be flushed)

Sampling position, per axis with size n = W or H, q = off / H, raw = ref + q:
    the division is good to 1 ulp (2u |q|; correctly rounded is inside), the add rounds once (u |raw|):
        E_l = e_in / H + 2u |q| + u |raw|
    clamp is 1-Lipschitz.  If raw <= -E_l or raw >= 1 + E_l the kernel clamps as the reference does and loc is 0 or 1
    EXACTLY; every later step is then exact too (2 loc - 1 = -+1, g + 1 = 0 or 2, 2n and 2n - 1 are integers below 2^24),
    so dp = 0.  Otherwise, with g = 2 loc - 1 and t = g + 1 (loc * 2 is exact; / 2 is exact):
        e_g  = 2 E_l + u (|g| + 2 E_l)                 lx * 2 - 1, one rounding with or without FMA
        e_t  = e_g + u (t + e_g)                       g + 1
        e_m  = n e_t + u n (t + e_t)                   (g + 1) * n ...
        e_s  = e_m + u (|n t - 1| + e_m)               ... - 1.  Contracted to one FMA the multiply's rounding drops out:
                                                       the uncontracted form is the larger and covers both
        dp   = e_s / 2
    dp is at most about n (E_l + 3.5 u): it scales with n and with max(|ref|, |off| / H).
The zero-padded interpolant is continuous and piecewise bilinear in (px, py), so moving the position by at most
(dpx, dpy) moves f_p by at most Sx dpx + Sy dpy, where Sx (Sy) is the largest |v(x1) - v(x0)| (|v(y1) - v(y0)|) over the
edges of the cells that the box [px +- dpx] x [py +- dpy] touches, for that channel, out-of-image taps counting as 0.
dp < 1/2 is asserted, so the box touches at most two cells per axis and stays inside the padded image.
    P_p = Sx dpx + Sy dpy

Blend.  The kernel forms wx1 = px - x0, wx0 = (x0 + 1) - px (one rounding each: px = -0.3 has more bits than 0.7 holds),
likewise in y, then w = wx wy aw (two multiplies), and accumulates the 32 weighted taps of a (token, head) with FMAs
(value times weight is not rounded on its own; bf16 values are exact in fp32).  A term passes at most 32 additions and
carries 4 weight roundings: gamma_36 < 37 u.  With A_p = the interpolant of |value| at the reference's position, the
kernel's own taps sum to at most A_p + P_p:
    E = sum_p aw_p P_p + sum_p e_aw_p (A_p + P_p) + 37 u sum_p aw_p (A_p + P_p)
fp32 output: E + 2^-126.  bf16 output: one round-to-nearest-even of the fp32 accumulator, `bf16_out_bound`.

add_pos is one correctly rounded fp32 add (and one round-to-nearest-even to bf16): no bound.  The result must equal the
CPU's x.float() + pos, cast with .bfloat16() for bf16, bit for bit, NaN positions included (`ref_add_pos`).

The `selector` kind needs no bound either: on `full_blocks` (H = 4, W = 8) with ref = (i + 0.5) / n, x offsets that are
multiples of H / W and integer y offsets, loc is a multiple of 1/n + 1/(2n), exact in fp32, px and py are exact integers,
and with logits 0 / -200 the chosen point's weight is exactly 1 (expf(-200) = 0 in fp32).  The output row of a (token,
head) is then one value row, bit for bit.  A target outside the image is reached by the clamp: loc = 0 or 1, px = -0.5 or
W - 0.5, half of the footprint outside, and the row is the border pixel's row times 1/2 per clamped axis - still exact.

`check` (depth_head_ref) asserts the elementwise bound and returns the two metrics of `train_node_ref.errors`.

Planted errors (`plant=`): a deliberately wrong copy of the reference.  A case that cannot show a plant raises
`NotExercised`; the CPU test proves `check` rejects each plant on at least one committed case.
"""
import collections

import torch
from torch.nn import functional as F

from depth_head_ref import NotExercised, TINY, U32, check  # noqa: F401  (check, NotExercised: re-exported)
from train_node_ref import errors  # noqa: F401
from transformer_gemm_ref import bf16_out_bound, bf16_rn, bf16_trunc, f32_out_bound  # noqa: F401

C = 256
NH, NP, CH = 8, 8, 32
SECOND = 1.0 + 2.0 ** -20      # room for the second-order terms of the first-order counts above
BLEND_ROUNDINGS = 32 + 5       # gamma_36 < 37 u

CORE_PLANTS = ("offset_y_over_W", "align_corners", "no_clamp", "border_padding", "ref_xy_swapped", "logits_of_next_head",
               "token_bias_not_on_logits", "token_bias_by_global_row", "head_major_read_as_nhwc",
               "odd_tail_takes_previous_token", "second_sample_reads_first", "bf16_truncated")
ADD_POS_PLANTS = ("pos_by_global_row", "bf16_truncated")

Case = collections.namedtuple("Case", "name B H W")
CASES = [Case("one_token", 1, 1, 1), Case("odd_9", 1, 3, 3), Case("odd_105_wide", 3, 5, 7), Case("tall", 2, 14, 9),
         Case("wide", 2, 9, 14), Case("full_blocks", 2, 4, 8), Case("very_wide", 1, 2, 33)]
BY_NAME = {c.name: c for c in CASES}
KINDS = ("random", "far", "big_logits")     # `selector` runs on full_blocks only, `nudged` in the non-finite test
OFF_SCALE = {"random": 6.0, "far": 50.0, "big_logits": 6.0, "nudged": 6.0}

Variant = collections.namedtuple("Variant", "name layout bf16 bias pts")
VARIANTS = [Variant("%s_%s%s" % (lay, "bf16" if bf else "f32", "_bias" if bias else ""), lay, bf, bias, None)
            for bias in (False, True) for lay in ("nhwc", "hm") for bf in (False, True)]
VARIANTS += [Variant("pts_shared", "nhwc", False, False, "shared"), Variant("pts_per_sample", "nhwc", False, False, "per_sample")]
VARIANT_BY_NAME = {v.name: v for v in VARIANTS}


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def to_head_major(value):
    """(B, H, W, 256) -> (B, 8, H*W, 32), what conv2d_nhwc(head_major=True) writes."""
    B, H, W, _ = value.shape
    return value.reshape(B, H * W, NH, CH).permute(0, 2, 1, 3).contiguous()


def grid_points(ref_x, ref_y):
    """(1, H*W, 2): the per-token (x, y) reference points of the grid form."""
    gy, gx = torch.meshgrid(ref_y, ref_x, indexing="ij")
    return torch.stack([gx, gy], -1).view(1, -1, 2)


def _nudge(off, ref, H, W):
    """Keeps every sampling position >= 0.02 px away from the bilinear kinks and 1e-4 away from the clamp edges."""
    B, N = off.shape[0], H * W
    o = off.double().view(B, N, NH * NP, 2)
    r = ref.double().view(-1, N, 1, 2)
    size = torch.tensor([W, H], dtype=torch.float64)
    for _ in range(8):
        loc = r + o.float().double() / H
        fr = loc * size - 0.5
        fr = fr - fr.floor()
        near = (fr < 0.02) | (fr > 0.98) | (loc.abs() < 1e-4) | ((loc - 1.0).abs() < 1e-4)
        o = torch.where(near, o + 0.05 * H / size, o)
    return o.view(off.shape).float()


def make_inputs(case, kind, variant):
    """dict: value (B,H,W,256) fp32|bf16 in NHWC order (the GPU test permutes it for head-major variants), ol (B,H,W,192)
    fp32 as handed to the kernel (with a bias variant: the problem's offsets_logits minus the bias, as the model splits
    it), ol_full (the undivided problem), token_bias (H*W,192) | None, ref_x (W), ref_y (H), ref_pts | None, variant.
    All variants of a (case, kind) share one problem.  Kinds: `random` (offsets randn x 6, logits randn x 2), `far`
    (offsets randn x 50, so nearly every point clamps), `big_logits` (randn x 30, one +88 per (token, head), every fifth
    (token, head) with 8 equal logits), `selector` (module docstring), `nudged` (`random`, kept off the kinks)."""
    B, H, W = case.B, case.H, case.W
    N = H * W
    g = _gen(case.name + "/" + kind)
    value = torch.randn(B, H, W, C, generator=g)
    if kind == "selector":
        assert case.name == "full_blocks"
        ref_x, ref_y = (torch.arange(W).float() + 0.5) / W, (torch.arange(H).float() + 0.5) / H
        off = (torch.randn(B, N, NH, NP, 2, generator=g) * 6.0)
        lg = torch.full((B, N, NH, NP), -200.0)
        pick = torch.randint(0, NP, (B, N, NH, 1), generator=g)
        tx = torch.randint(-2, W + 2, (B, N, NH), generator=g)
        ty = torch.randint(-2, H + 2, (B, N, NH), generator=g)
        tok = torch.arange(N).view(1, N, 1)
        sel = torch.stack([(tx - tok % W).float() * (float(H) / W), (ty - tok // W).float()], -1)   # (B,N,NH,2)
        off.scatter_(3, pick[..., None].expand(B, N, NH, 1, 2), sel[:, :, :, None, :])
        lg.scatter_(3, pick, 0.0)
        ol = torch.cat([off.reshape(B, N, 128), lg.reshape(B, N, 64)], -1).reshape(B, H, W, 192)
        target = dict(pick=pick[..., 0], tx=tx, ty=ty)
    else:
        ref_x, ref_y = torch.linspace(0, 1, W), torch.linspace(0, 1, H)
        off = torch.randn(B, H, W, 128, generator=g) * OFF_SCALE[kind]
        if kind == "far":   # point 7 of every head stays near its reference point: the interior is still visited
            off.view(B, N, NH, NP, 2)[:, :, :, NP - 1] *= 1.0 / OFF_SCALE[kind]
        lg = torch.randn(B, H, W, 64, generator=g) * (30.0 if kind == "big_logits" else 2.0)
        if kind == "big_logits":
            l4 = lg.view(B, N, NH, NP)
            top = torch.randint(0, NP, (B, N, NH, 1), generator=g)
            l4.scatter_(3, top, 88.0)
            flat = l4.view(B * N * NH, NP)
            flat[::5] = flat[::5, :1].clone()                          # every fifth (token, head): 8 equal logits
        target = None
    pts = None
    if variant.pts == "shared":
        pts = grid_points(ref_x, ref_y)
    elif variant.pts == "per_sample":
        pts = torch.rand(B, N, 2, generator=_gen(case.name + "/" + kind + "/pts")) * 1.4 - 0.2
        pts[:, 0, 0], pts[:, N - 1, 1] = -0.15, 1.1          # outside [0, 1] on either side, whatever was drawn
    if kind == "nudged":
        off = _nudge(off, grid_points(ref_x, ref_y) if pts is None else pts, H, W).view(B, H, W, 128)
    if kind != "selector":
        ol = torch.cat([off, lg], -1).contiguous()
    tb = None
    ol_full = ol
    if variant.bias:
        tb = torch.randn(N, 192, generator=_gen(case.name + "/" + kind + "/bias"))
        tb[:, :128] *= 3.0
        ol = (ol_full - tb.view(1, H, W, 192)).contiguous()
    if variant.bf16:
        value = value.bfloat16()
    return dict(value=value, ol=ol, ol_full=ol_full, token_bias=tb, ref_x=ref_x, ref_y=ref_y, ref_pts=pts, variant=variant,
                target=target)


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
def _taps(v, b_idx, h_idx, yi, xi, H, W, border=False):
    """v (B,H,W,NH,CH) fp64; yi, xi (B,N,NH,NP) integer pixel coordinates, any value: the (B,N,NH,NP,CH) rows, zero
    outside the image (the clamped pixel with `border`).  An out-of-image tap is never multiplied: it is 0."""
    ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    rows = v[b_idx, yi.clamp(0, H - 1), xi.clamp(0, W - 1), h_idx]
    return rows if border else torch.where(ok[..., None], rows, rows.new_zeros(()))


def _bilinear(v, b_idx, h_idx, px, py, H, W, border=False):
    x0, y0 = torch.floor(px), torch.floor(py)
    wx1, wy1 = (px - x0)[..., None], (py - y0)[..., None]
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    xi, yi = x0.long(), y0.long()
    t = lambda dy, dx: _taps(v, b_idx, h_idx, yi + dy, xi + dx, H, W, border)  # noqa: E731
    return wy0 * (wx0 * t(0, 0) + wx1 * t(0, 1)) + wy1 * (wx0 * t(1, 0) + wx1 * t(1, 1))


def _slopes(v, b_idx, h_idx, px, py, dpx, dpy, H, W):
    """Sx, Sy (B,N,NH,NP,CH): the largest edge difference over the cells that the box [p +- dp] touches."""
    Sx = Sy = None
    for cx in (torch.floor(px - dpx), torch.floor(px + dpx)):
        for cy in (torch.floor(py - dpy), torch.floor(py + dpy)):
            xi, yi = cx.long().clamp(-1, W - 1), cy.long().clamp(-1, H - 1)
            t = lambda dy, dx: _taps(v, b_idx, h_idx, yi + dy, xi + dx, H, W)  # noqa: E731
            v00, v01, v10, v11 = t(0, 0), t(0, 1), t(1, 0), t(1, 1)
            sx = torch.maximum((v01 - v00).abs(), (v11 - v10).abs())
            sy = torch.maximum((v10 - v00).abs(), (v11 - v01).abs())
            Sx = sx if Sx is None else torch.maximum(Sx, sx)
            Sy = sy if Sy is None else torch.maximum(Sy, sy)
    return Sx, Sy


def _position(ref, off, e_off, n, H, clamp=True):
    """One axis.  ref (B,N,1,1), off, e_off (B,N,NH,NP), n = the axis' size.  Returns (loc, dp, raw)."""
    q = off / H
    raw = ref + q
    E_l = (e_off / H + 2.0 * U32 * q.abs() + U32 * raw.abs()) * SECOND
    if not clamp:
        return raw, None, raw
    loc = raw.clamp(0.0, 1.0)
    g, t = 2.0 * loc - 1.0, 2.0 * loc
    e_g = 2.0 * E_l + U32 * (g.abs() + 2.0 * E_l)
    e_t = e_g + U32 * (t + e_g)
    e_m = n * e_t + U32 * n * (t + e_t)
    e_s = e_m + U32 * ((n * t - 1.0).abs() + e_m)
    exact = (raw <= -E_l) | (raw >= 1.0 + E_l)
    dp = torch.where(exact, torch.zeros_like(raw), 0.5 * e_s * SECOND)
    return loc, dp, raw


Deform = collections.namedtuple("Deform", "out bound aw px py dpx dpy raw_x raw_y pos_share")


def ref_deform_attn(case, ins, plant=None, input_err=None):
    """The unrounded fp64 output in the kernel's output shape ((B,H,W,256); (B,H*W,256) for the pts variants) and the
    elementwise bound of the kernel's fp32 or bf16 output.  input_err (B,H,W,192) >= 0: a perturbation of offsets_logits
    the bound has to absorb on top of the kernel's own arithmetic."""
    if plant is not None and plant not in CORE_PLANTS:
        raise ValueError(plant)
    var = ins["variant"]
    B, H, W = case.B, case.H, case.W
    N = H * W
    rows = B * N
    ol = ins["ol"].double().reshape(B, N, 192)
    tb = ins["token_bias"]
    e_in = torch.zeros_like(ol) if input_err is None else input_err.double().reshape(B, N, 192).clone()
    if plant in ("token_bias_not_on_logits", "token_bias_by_global_row") and tb is None:
        raise NotExercised("no token_bias")
    full = ol
    if tb is not None:
        add = tb.double()[None].expand(B, N, 192)
        if plant == "token_bias_by_global_row":   # the table read at b*T + t: past its end (zeros) for every later sample
            if B == 1:
                raise NotExercised("one sample")
            add = torch.cat([add[:1], torch.zeros_like(add[1:])], 0)
        if plant == "token_bias_not_on_logits":
            add = torch.cat([add[..., :128], torch.zeros_like(add[..., 128:])], -1)
        full = ol + add
        e_in = e_in + U32 * full.abs() * SECOND
    off = full[..., :128].reshape(B, N, NH, NP, 2)
    e_off = e_in[..., :128].reshape(B, N, NH, NP, 2)
    lg = full[..., 128:].reshape(B, N, NH, NP)
    e_lg = e_in[..., 128:].reshape(B, N, NH, NP)
    if plant == "logits_of_next_head":
        lg = torch.roll(lg, -1, 2)
    if ins["ref_pts"] is not None:
        pts = ins["ref_pts"].double()
        if plant == "second_sample_reads_first":
            if var.pts != "per_sample" or B == 1:
                raise NotExercised("needs per-sample reference points and a second sample")
            pts = pts[:1]
        pts = pts.expand(B, N, 2)
    else:
        if plant == "second_sample_reads_first":
            raise NotExercised("no ref_pts")
        pts = grid_points(ins["ref_x"].double(), ins["ref_y"].double()).expand(B, N, 2)
    if plant == "ref_xy_swapped":
        if torch.equal(pts, pts.flip(-1)):
            raise NotExercised("x and y reference points coincide")
        pts = pts.flip(-1)
    rx, ry = pts[..., 0].reshape(B, N, 1, 1), pts[..., 1].reshape(B, N, 1, 1)
    # softmax
    mx = lg.amax(-1, keepdim=True)
    aw = torch.softmax(lg, -1)
    eps = (e_lg + U32 * (lg - mx).abs()).amax(-1, keepdim=True)
    e_aw = aw * (torch.expm1(2.0 * eps) + 16.0 * U32) * SECOND + TINY
    # positions
    if plant == "offset_y_over_W" and H == W:
        raise NotExercised("H == W")
    clamp = plant != "no_clamp"
    loc_x, dpx, raw_x = _position(rx, off[..., 0], e_off[..., 0], float(W), float(H), clamp)
    loc_y, dpy, raw_y = _position(ry, off[..., 1], e_off[..., 1], float(H), float(W if plant == "offset_y_over_W" else H),
                                  clamp)
    if not clamp:
        if not bool(((raw_x < 0) | (raw_x > 1) | (raw_y < 0) | (raw_y > 1)).any()):
            raise NotExercised("no point is clamped")
        dpx, dpy = torch.zeros_like(raw_x), torch.zeros_like(raw_y)
    if plant == "align_corners":
        px, py = loc_x * (W - 1), loc_y * (H - 1)
    else:
        px, py = loc_x * W - 0.5, loc_y * H - 0.5
    assert float(dpx.max()) < 0.5 and float(dpy.max()) < 0.5
    # the gather
    value = ins["value"]
    if plant == "head_major_read_as_nhwc":
        if var.layout != "hm":
            raise NotExercised("NHWC values")
        value = to_head_major(value).reshape(B, H, W, C)    # the head-major buffer under NHWC strides
    v = value.double().reshape(B, H, W, NH, CH)
    b_idx = torch.arange(B).view(B, 1, 1, 1).expand(B, N, NH, NP)
    h_idx = torch.arange(NH).view(1, 1, NH, 1).expand(B, N, NH, NP)
    border = plant == "border_padding"
    if border and not bool(((px < 0) | (px > W - 1) | (py < 0) | (py > H - 1)).any()):
        raise NotExercised("no footprint leaves the image")
    f = _bilinear(v, b_idx, h_idx, px, py, H, W, border)                 # (B,N,NH,NP,CH)
    A = _bilinear(v.abs(), b_idx, h_idx, px, py, H, W)
    Sx, Sy = _slopes(v, b_idx, h_idx, px, py, dpx, dpy, H, W)
    P = Sx * dpx[..., None] + Sy * dpy[..., None]
    w = aw[..., None]
    out = (w * f).sum(3)                                                 # (B,N,NH,CH)
    pos = (w * P).sum(3)
    E = pos * SECOND + (e_aw[..., None] * (A + P)).sum(3) + BLEND_ROUNDINGS * U32 * (w * (A + P)).sum(3)
    if plant == "odd_tail_takes_previous_token":
        if rows % 2 == 0 or rows == 1:
            raise NotExercised("no odd tail besides token 0's")
        out = out.reshape(rows, NH, CH).clone()
        out[rows - 1] = out[rows - 2]
    if plant == "bf16_truncated":
        if not var.bf16:
            raise NotExercised("fp32 output is not rounded")
        out = bf16_trunc(out)
    shape = (B, N, C) if var.pts else (B, H, W, C)
    out, E = out.reshape(shape), E.reshape(shape)
    bound = bf16_out_bound(out, E) if var.bf16 else f32_out_bound(E)
    share = float(pos.sum() / E.sum().clamp_min(1e-300))
    return Deform(out, bound, aw, px, py, dpx, dpy, raw_x, raw_y, share)


def selector_expectation(case, ins):
    """Integer arithmetic only: (pixel index (B,N,NH), scale (B,N,NH)) of the value row each (token, head) selects; a
    target outside the image is clamped to the border pixel at half weight per clamped axis."""
    t = ins["target"]
    H, W = case.H, case.W
    tx, ty = t["tx"], t["ty"]
    cx, cy = tx.clamp(0, W - 1), ty.clamp(0, H - 1)
    scale = torch.where(tx == cx, 1.0, 0.5) * torch.where(ty == cy, 1.0, 0.5)
    return cy * W + cx, scale.double()


def selector_rows(case, ins):
    """The expected output (B,H,W,256) in value's dtype, gathered: no floating-point arithmetic besides the exact scale."""
    B, H, W = case.B, case.H, case.W
    N = H * W
    pix, scale = selector_expectation(case, ins)
    v = ins["value"].reshape(B, N, NH, CH)
    rows = v[torch.arange(B).view(B, 1, 1), pix, torch.arange(NH).view(1, 1, NH)]           # (B,N,NH,CH)
    return (rows.double() * scale[..., None]).to(ins["value"].dtype).reshape(B, H, W, C)


def grid_sample_composition(value, ol, ref, H, W):
    """The F.grid_sample composition of the sampling core (core_torch of tests/test_deform_attn_grad_gpu.py, restated).
    value (B, N, 256), ol (B, N, 192), ref (B, N, 2) -> (B, N, 256)."""
    B, N, _ = value.shape
    off = ol[..., :128].reshape(B, N, 8, 8, 2)
    aw = ol[..., 128:].reshape(B, N, 8, 8).softmax(-1)
    loc = (ref[:, :, None, None, :] + off / H).clamp(0, 1)
    v = value.reshape(B, H, W, 8, 32).permute(0, 3, 4, 1, 2).reshape(B * 8, 32, H, W)
    grid = (loc * 2.0 - 1.0).permute(0, 2, 1, 3, 4).reshape(B * 8, N, 8, 2)
    s = F.grid_sample(v, grid, mode="bilinear", align_corners=False)
    w = aw.permute(0, 2, 1, 3).reshape(B * 8, 1, N, 8)
    return (s * w).sum(-1).view(B, 8, 32, N).permute(0, 3, 1, 2).reshape(B, N, 256)


# ----------------------------------------------------------------------------------------------------------------------
# add_pos
# ----------------------------------------------------------------------------------------------------------------------
ADD_POS_ROWS = (1, 3, 5, 257)
ADD_POS_B = (1, 3)


def make_add_pos_inputs(T, B, bf16):
    """x (B, T, 256) fp32|bf16, pos (T, 256) fp32, with +-0, a NaN, +-inf and bf16 ties among them."""
    g = _gen("add_pos/%d/%d" % (T, B))
    x = torch.randn(B, T, C, generator=g)
    pos = torch.randn(T, C, generator=g)
    x[0, 0, :8] = torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1.0, 1.0, -3.0])
    pos[0, :8] = torch.tensor([-0.0, -0.0, 1.0, 1.0, float("inf"), 2.0 ** -8, 3 * 2.0 ** -8, -3 * 2.0 ** -7])
    # 1 + 2^-8 ties to 1 (even); 1 + 3 * 2^-8 ties up to 1 + 2^-6; -3 - 3 * 2^-7 ties to -3 - 2^-5
    x[B - 1, T - 1, 250:] = torch.tensor([float("nan"), 0.0, float("inf"), 1.0, -1.0, 2.0])
    pos[T - 1, 250:] = torch.tensor([0.0, float("nan"), float("-inf"), -1.0, 1.0, 2.0 ** -7])
    return (x.bfloat16() if bf16 else x), pos


def ref_add_pos(x, pos, plant=None):
    """The CPU's correctly rounded x.float() + pos[t], in x's dtype (round to nearest even for bf16)."""
    if plant is not None and plant not in ADD_POS_PLANTS:
        raise ValueError(plant)
    B, T = x.shape[0], pos.shape[0]
    p = pos.view(1, T, C).expand(B, T, C)
    if plant == "pos_by_global_row":
        if B == 1:
            raise NotExercised("one sample")
        p = torch.cat([p[:1], torch.zeros_like(p[1:])], 0)
    s = x.float().reshape(B, T, C) + p
    if x.dtype == torch.bfloat16:
        if plant == "bf16_truncated":
            return (s.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16().reshape(x.shape)
        return s.bfloat16().reshape(x.shape)
    if plant == "bf16_truncated":
        raise NotExercised("fp32 output is not rounded")
    return s.reshape(x.shape)


def same_bits(a, b):
    """torch.equal with NaN compared by position (and +0 == -0, as torch.equal has it)."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


# ----------------------------------------------------------------------------------------------------------------------
# float32 emulation of deform_attn_kernel, operation by operation
# ----------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate_f32(case, ins, contract):
    """csrc/bev_transformer.hip deform_attn_kernel in float32 torch arithmetic.  contract: (gx + 1) * W - 1 as one FMA."""
    var = ins["variant"]
    B, H, W = case.B, case.H, case.W
    N = H * W
    one = torch.tensor(1.0, dtype=torch.float32)
    ol = ins["ol"].reshape(B, N, 192)
    if ins["token_bias"] is not None:
        ol = ol + ins["token_bias"][None]
    assert ol.dtype == torch.float32
    off = ol[..., :128].reshape(B, N, NH, NP, 2)
    lg = ol[..., 128:].reshape(B, N, NH, NP)
    mx = lg.amax(-1, keepdim=True)
    e = torch.exp(lg - mx)
    pair = e[..., 0::2] + e[..., 1::2]                        # the lane's own two points
    s2 = pair[..., 0::2] + pair[..., 1::2]                    # xor 1
    tot = (s2[..., 0] + s2[..., 1])[..., None]                # xor 2
    aw = e / tot
    pts = ins["ref_pts"] if ins["ref_pts"] is not None else grid_points(ins["ref_x"], ins["ref_y"])
    pts = pts.expand(B, N, 2)
    fH, fW = torch.tensor(float(H)), torch.tensor(float(W))

    def axis(r, o, n):
        l = (r + o / fH).clamp(0.0, 1.0)
        gcoord = l * 2.0 - 1.0
        t = gcoord + 1.0
        p = (_fma32(t, n.expand_as(t), -one.expand_as(t)) if contract else t * n - 1.0) / 2.0
        p0 = torch.floor(p)
        return p0.long(), p - p0, (p0 + 1.0) - p

    x0, wx1, wx0 = axis(pts[..., 0].reshape(B, N, 1, 1), off[..., 0], fW)
    y0, wy1, wy0 = axis(pts[..., 1].reshape(B, N, 1, 1), off[..., 1], fH)
    v = ins["value"].float().reshape(B, H, W, NH, CH)
    b_idx = torch.arange(B).view(B, 1, 1).expand(B, N, NH)
    h_idx = torch.arange(NH).view(1, 1, NH).expand(B, N, NH)
    acc = torch.zeros(B, N, NH, CH)
    for p in range(NP):
        for dy, dx, wy, wx in ((0, 0, wy0, wx0), (0, 1, wy0, wx1), (1, 0, wy1, wx0), (1, 1, wy1, wx1)):
            xi, yi = x0[..., p] + dx, y0[..., p] + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            wgt = torch.where(ok, wx[..., p] * wy[..., p] * aw[..., p], torch.zeros(()))
            rows = v[b_idx, yi.clamp(0, H - 1), xi.clamp(0, W - 1), h_idx]
            acc = _fma32(rows, wgt[..., None].expand_as(rows), acc)
    assert acc.dtype == torch.float32
    out = acc.reshape((B, N, C) if var.pts else (B, H, W, C))
    return out.bfloat16() if var.bf16 else out
