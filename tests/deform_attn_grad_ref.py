"""fp64 reference, DERIVED error bounds, cases and planted errors for the tests of the deformable-attention BACKWARD alone
(csrc/deform_grad.hip through ops.deform_attn_bwd and the C entry lss_deform_attn_bwd: tests/test_deform_attn_bwd_gpu.py on
the GPU, tests/test_deform_attn_grad_ref_cpu.py for this helper itself).  The forward's helper is tests/deform_attn_ref.py;
its cases, inputs, position model (`_position`: loc, dp, raw) and softmax-weight bound are reused here.

Everything is fp64 on the CPU.  u = 2^-24.  No bound is measured on a kernel.

The operation.  Inputs value (B,N,256), ol (B,N,192) = [offsets (head, point, xy) | logits (head, point)], ref_pts (1|B,N,2),
d_out (B,N,256).  Per (sample, token, head), over its 8 points p and the head's 32 channels c, with the forward's aw, loc,
px = loc_x W - 1/2, py = loc_y H - 1/2, x0 = floor(px), y0 = floor(py), wx1 = px - x0, wx0 = 1 - wx1 (likewise y) and
v00..v11 the zero-padded taps of the cell (x0, y0), and with the dots d_ij = sum_c d_out_c v_ij,c:
    G_p   = wy0 (wx0 d00 + wx1 d01) + wy1 (wx0 d10 + wx1 d11)
    PX_p  = wy0 (d01 - d00) + wy1 (d11 - d10),    PY_p = wx0 (d10 - d00) + wx1 (d11 - d01)
    dlogit_p = aw_p (G_p - sum_q aw_q G_q)
    d offx_p = mx aw_p PX_p W / H,   d offy_p = my aw_p PY_p       (BOTH offsets are divided by H in the forward)
    mx, my = 1 where 0 <= raw <= 1, INCLUSIVE (torch.clamp's backward); the derivative is taken in the cell
    [floor(px), floor(px) + 1): at an integer px it is the cell to the right (what grid_sample's backward returns)
    d_value[b, cell, head, c] = sum over every (token, point, tap landing on the cell) of aw_p w_tap d_out[token, head, c]
The weight a point gives a fixed cell (x, y) is aw hx hy with the hat hx = max(0, 1 - |px - x|): the same four taps.

Bounds.  From the forward helper: e_aw = aw (expm1(2 eps) + 16 u) + 2^-126 with eps = max_p u |logit_p - max| (both the
gather and the scatter kernel form the forward's softmax), the position error dp per axis, and
E_l = 2u |off / H| + u |raw| for the unclamped location.  SECOND = 1 + 2^-20 makes room for second-order terms.

d_value, per element.  The scatter kernel forms its own position p' (|p' - p| <= dp), wx = fl(px' - x0') and
fl((x0' + 1) - px') (one rounding each), w = fl(fl(wx wy) aw): 4 roundings on hx(px') hy(py') aw'.  The hat is continuous and
1-Lipschitz across the kinks, so for ANY cell, whichever side of a kink the kernel falls on,
    |hx(px') hy(py') - hx hy| <= tx Hy + hx ty,     Hx = the largest hat over the box [px +- dpx] (likewise Hy),
                                                    tx = dpx where Hx > 0, else 0 (likewise ty)
and the term is spread over the up to 4 x 4 cells (x0 - 1 .. x0 + 2) that the box can give weight to.  One contribution's
error is |d_out_c| A, A = aw (tx Hy + hx ty) + (e_aw + 4u aw + 2^-126) Hx Hy.  Each add is the product rounded to the
sample's fixed-point step, 2^(e - F), max finite |d_out| < 2^e, F = min(62 - ceil(log2 N), 50): n_adds(cell) 2^(e - F - 1),
n_adds = the number of points with Hx Hy > 0 for the cell (a tap of weight exactly 0 adds an exact 0).  The integer sum is
exact; int64 -> double -> float is one fp32 rounding (the 2^-53 of the first step is inside SECOND):
    E_value = sum |d_out_c| A + n_adds 2^(e - F - 1) + u (|ref| + that) + 2^-126

d_ol.  The gather kernel dots d_out with each tap over a lane's 8 channels (a product and three additions), blends, and sums
the quad's 4 lanes (2 additions).  Counting every rounding a term can pass, the weights' own included: 12 for G (4 dot +
2 weights + 4 blend + 2 quad), 10 for PX and PY: gamma_12 < 13 u, times the magnitude sums
    MG = max_taps a_ij,  MPX = max(a00 + a01, a10 + a11),  MPY = max(a00 + a10, a01 + a11),  a_ij = sum_c |d_out_c v_ij,c|
(the kernel's weights are in [0, 1] and sum to 1 per axis).  G is the zero-padded bilinear interpolant of the dot field:
continuous, so it moves by at most SGx dpx + SGy dpy, SGx = max(|d01 - d00|, |d11 - d10|), SGy likewise, over the cells the
box touches.  PX is piecewise CONSTANT in px and, in a fixed column of cells, continuous and piecewise linear in py with
slope X = |d11 - d10 - d01 + d00|; PY the other way round with the same X.  Where the box [px +- dpx] holds an integer the
kernel may stand in the other column: the bound then adds |PX_other(py) - PX(py)|, the difference of the two one-sided
values (likewise PY / py), and every maximum above runs over both cells.  Where raw lies within E_l of 0 or 1 the kernel's
mask may be the other one: the bound then adds |aw PX W / H| (|aw PY|).  No point is left out of the comparison; the share
of points widened in either way is returned and the CPU test caps it at 1 %.
    dG  = SGx dpx + SGy dpy + 13u MG,   dPX = [side] + X dpy + 13u MPX,   dPY = [side] + X dpx + 13u MPY
    d offx = mx fl(fl(aw' PX') fl(W / H)): 3 more roundings
        E_offx = (W / H) ((e_aw + 3u aw)(|PX| + dPX) + aw dPX) + [mask] + 4 max(1, W / H) 2^-126      (0 where mx is surely 0)
    s = sum_q aw_q G_q (4 roundings: 5u):   ds = sum_q (e_aw_q (|G_q| + dG_q) + aw_q dG_q) + 5u sum_q (aw_q + e_aw_q)(|G_q| + dG_q)
    dlogit = fl(aw' fl(G' - s')):  E_logit = (e_aw + 2u aw)(|G - s| + dG + ds) + aw (dG + ds) + 2^-126

Kinds.  `random`, `far`, `big_logits` (saturates the softmax Jacobian) and `nudged` are the forward helper's; `skewed` is
`random` with sample b's d_out scaled by 2^(-44 b), so that a fixed-point step taken from the batch maximum would flush
sample 1; `exact` (module function `_make_exact`) makes every fp32 operation exact, and the kernel's outputs then equal the
reference bit for bit.  Each kind runs with the shared grid (batch stride 0) and with per-sample reference points.

How much slack the bounds carry: the largest max(bound) / max|ref| per output over the committed (case, kind, points)
(printed by test_emulation_is_inside_the_bound, `report`ed by the GPU test as `bound_over_max`):
    d_value    4.3e-5  (tiles_2x3 big_logits per_sample; tall random shared: 1.3e-5)
    d offsets  0.49    (tiles_2x3 skewed per_sample: ONE widened point, whose bound is the difference of its two one-sided
                       derivatives; a case without a widened point, tall random shared: 6.0e-6)
    d logits   3.7e-3  (one_token big_logits per_sample; 6.0e-4 on very_wide big_logits; tall random shared: 6.0e-5).  On
                       one_token big_logits shared the saturated softmax makes max|ref| itself 1e-25: the ratio means nothing
The largest error / bound the fp32 emulation reaches: d_value 0.93 (one add of 1.47 steps rounded to 1 step: the half-step
term is attained), d offsets 0.0 .. 1.0 (1.0 where the emulation stands on the other side of a kink), d logits 0.20.

Planted errors (`plant=`): a deliberately wrong copy of the reference; a case that cannot show it raises `NotExercised`.
"""
import collections
import math

import torch

from deform_attn_ref import (CASES, CH, NH, NP, SECOND, TINY, U32, VARIANT_BY_NAME, Case, NotExercised, _bilinear,  # noqa: F401
                             _fma32, _gen, _position, _taps, check, grid_points, make_inputs)

C = 256
DOT_ROUNDINGS = 12 + 1          # gamma_12 < 13 u
GCASES = list(CASES) + [Case("tiles_2x3", 2, 19, 35), Case("pow2", 2, 8, 16)]
BY_NAME = {c.name: c for c in GCASES}
KINDS = ("random", "far", "big_logits", "nudged", "skewed")
EXACT_CASES = ("full_blocks", "pow2")
PTS = ("shared", "per_sample")
TS, RAD = 16, 9                 # the scatter kernel's token tile and window margin
WIDENED_CAP = 0.01

PLANTS = ("doffx_without_W_over_H", "doffy_times_W_over_H", "offset_y_over_W", "clamp_mask_exclusive", "clamp_mask_ignored",
          "left_derivative_at_kink", "border_padding_in_derivative", "dlogit_without_mean_term", "logits_of_next_head",
          "ref_xy_swapped", "second_sample_reads_first_ref", "dvalue_cell_index_H_W_swapped", "dvalue_far_taps_dropped",
          "odd_tail_takes_previous_token", "scale_from_whole_batch")


def ceil_log2(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


def fx_bits(N):
    """F of the file comment of deform_grad.hip."""
    return min(62 - ceil_log2(N), 50)


def fx_exponents(d_out):
    """e per sample: the largest finite |d_out| < 2^e (0 for an all-zero sample), as frexpf has it."""
    a = d_out.detach().double().abs().reshape(d_out.shape[0], -1)
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return [math.frexp(float(m))[1] for m in a.amax(1)]


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def _make_exact(case, pts):
    """Module docstring, `exact`: small-integer value, d_out = small integers x one power of two per (token, head), two
    points per (token, head) at logit 0 and six at -200 (weights 1/2, 1/2, 0 in fp32), the two on targets drawn from:
    outside the image (mask 0), the half-pixels -1/2 and n - 1/2 (raw exactly 0 or 1, mask 1), every integer pixel centre
    (x0 = W - 1 and y0 = H - 1 included: the derivative's second tap is out of the image).  H / W is a power of two."""
    assert case.name in EXACT_CASES
    B, H, W = case.B, case.H, case.W
    N = H * W
    g = _gen(case.name + "/exact")
    value = torch.randint(-3, 4, (B, N, C), generator=g).float()
    d_out = (torch.randint(-4, 5, (B, N, NH, CH), generator=g).float()
             * 2.0 ** torch.randint(-3, 4, (B, N, NH, 1), generator=g).float()).reshape(B, N, C)
    off = torch.randn(B, N, NH, NP, 2, generator=g) * 6.0
    lg = torch.full((B, N, NH, NP), -200.0)
    pick = torch.rand(B, N, NH, NP, generator=g).argsort(-1)[..., :2]                     # two distinct points
    doubled = lambda n: torch.tensor([-4, -2, -1] + list(range(0, 2 * n, 2)) + [2 * n - 1, 2 * n, 2 * n + 2])  # noqa: E731
    xs, ys = doubled(W), doubled(H)
    tx2 = xs[torch.randint(0, len(xs), (B, N, NH, 2), generator=g)]                       # twice the target coordinate
    ty2 = ys[torch.randint(0, len(ys), (B, N, NH, 2), generator=g)]
    tok = torch.arange(N).view(1, N, 1, 1)
    sel = torch.stack([(tx2.float() / 2 - (tok % W).float()) * (float(H) / W), ty2.float() / 2 - (tok // W).float()], -1)
    off.scatter_(3, pick[..., None].expand(B, N, NH, 2, 2), sel)
    lg.scatter_(3, pick, 0.0)
    ol = torch.cat([off.reshape(B, N, 128), lg.reshape(B, N, 64)], -1).contiguous()
    ref = grid_points((torch.arange(W).float() + 0.5) / W, (torch.arange(H).float() + 0.5) / H)
    if pts == "per_sample":
        ref = ref.expand(B, N, 2).contiguous()
    return dict(value=value, ol=ol, ref_pts=ref, d_out=d_out, kind="exact", pts=pts, target=dict(pick=pick, tx2=tx2, ty2=ty2))


def exact_edge_sets(case, ins):
    """Boolean (B,N,NH,NP,2) over the offsets of an `exact` problem: the chosen points' axes whose target is a half-pixel
    (raw exactly 0 or 1: mask 1), and those whose target is outside the image (mask 0)."""
    B, N = case.B, case.H * case.W
    t = ins["target"]
    on_edge = torch.zeros(B, N, NH, NP, 2, dtype=torch.bool)
    outside = torch.zeros(B, N, NH, NP, 2, dtype=torch.bool)
    for a, (t2, n) in enumerate(((t["tx2"], case.W), (t["ty2"], case.H))):
        on_edge[..., a].scatter_(3, t["pick"], (t2 == -1) | (t2 == 2 * n - 1))
        outside[..., a].scatter_(3, t["pick"], (t2 < -1) | (t2 > 2 * n - 1))
    return on_edge, outside


def make_grad_inputs(case, kind, pts):
    """dict: value (B,N,256), ol (B,N,192), ref_pts (1,N,2) for `shared` | (B,N,2), d_out (B,N,256), all fp32.  value,
    ol and ref_pts are the forward helper's problem of the same (case, kind); d_out is randn from the case's own generator."""
    assert pts in PTS
    if kind == "exact":
        return _make_exact(case, pts)
    B, N = case.B, case.H * case.W
    ins = make_inputs(case, "random" if kind == "skewed" else kind, VARIANT_BY_NAME["pts_" + pts])
    d_out = torch.randn(B, N, C, generator=_gen(case.name + "/" + kind + "/d_out"))
    if kind == "skewed":
        d_out = d_out * (2.0 ** (-44.0 * torch.arange(B, dtype=torch.float32))).view(B, 1, 1)
    return dict(value=ins["value"].reshape(B, N, C), ol=ins["ol"].reshape(B, N, 192).contiguous(), ref_pts=ins["ref_pts"],
                d_out=d_out, kind=kind, pts=pts, target=None)


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
Grad = collections.namedtuple("Grad", "d_value d_ol bound_value bound_ol widened aw px py raw_x raw_y mask_x mask_y n_far "
                              "n_adds")


def _cell(v, g, b_idx, h_idx, yi, xi, H, W, border=False):
    """The dots of g with the four taps (00, 01, 10, 11) of the cell whose top-left pixel is (xi, yi): (..., 4) signed and
    (..., 4) of magnitudes.  g broadcasts against the taps' (..., CH)."""
    d, a = [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        prod = g * _taps(v, b_idx, h_idx, yi + dy, xi + dx, H, W, border)
        d.append(prod.sum(-1))
        a.append(prod.abs().sum(-1))
    return torch.stack(d, -1), torch.stack(a, -1)


def _blend(d, wx0, wx1, wy0, wy1):
    G = wy0 * (wx0 * d[..., 0] + wx1 * d[..., 1]) + wy1 * (wx0 * d[..., 2] + wx1 * d[..., 3])
    PX = wy0 * (d[..., 1] - d[..., 0]) + wy1 * (d[..., 3] - d[..., 2])
    PY = wx0 * (d[..., 2] - d[..., 0]) + wx1 * (d[..., 3] - d[..., 1])
    return G, PX, PY


def _cell_maxima(d, a):
    """SGx, SGy, X, MG, MPX, MPY of one cell (module docstring)."""
    d00, d01, d10, d11 = d.unbind(-1)
    a00, a01, a10, a11 = a.unbind(-1)
    return [torch.maximum((d01 - d00).abs(), (d11 - d10).abs()), torch.maximum((d10 - d00).abs(), (d11 - d01).abs()),
            (d11 - d10 - d01 + d00).abs(), a.amax(-1), torch.maximum(a00 + a01, a10 + a11), torch.maximum(a00 + a10, a01 + a11)]


def _E_l(raw, off, H):
    q = off / H
    return (2.0 * U32 * q.abs() + U32 * raw.abs()) * SECOND


def ref_deform_grad(case, ins, plant=None, bounds=True, tokens=None, d_out=None):
    """The unrounded fp64 d_value (B,N,256) and d_ol (B,T,192) with their elementwise bounds (None with bounds=False).
    tokens (LongTensor of T token ids; default all N): only these tokens sample - ol, ref_pts and d_out are read at these
    rows, d_ol has these rows, and d_value (with its bound) holds their contributions alone.  d_out overrides ins'."""
    if plant is not None and plant not in PLANTS:
        raise ValueError(plant)
    B, H, W = case.B, case.H, case.W
    N = H * W
    tok = torch.arange(N) if tokens is None else tokens.long()
    T = tok.numel()
    rWH = float(W) / float(H)
    square = H == W
    d_out = ins["d_out"] if d_out is None else d_out
    ol = ins["ol"].double().reshape(B, N, 192)[:, tok]
    off = ol[..., :128].reshape(B, T, NH, NP, 2)
    lg = ol[..., 128:].reshape(B, T, NH, NP)
    g = d_out.double().reshape(B, N, NH, 1, CH)[:, tok]
    if plant == "logits_of_next_head":
        lg = torch.roll(lg, -1, 2)
    pts = ins["ref_pts"].double()
    if plant == "second_sample_reads_first_ref":
        if B == 1 or pts.shape[0] == 1 or all(torch.equal(pts[0], pts[b]) for b in range(1, B)):
            raise NotExercised("needs a second sample with reference points of its own")
        pts = pts[:1]
    pts = pts.expand(B, N, 2)[:, tok]
    if plant == "ref_xy_swapped":
        if torch.equal(pts, pts.flip(-1)):
            raise NotExercised("x and y reference points coincide")
        pts = pts.flip(-1)
    if plant in ("doffx_without_W_over_H", "doffy_times_W_over_H", "offset_y_over_W", "dvalue_cell_index_H_W_swapped") and square:
        raise NotExercised("H == W")
    rx, ry = pts[..., 0].reshape(B, T, 1, 1), pts[..., 1].reshape(B, T, 1, 1)
    # the forward's softmax and positions
    aw = torch.softmax(lg, -1)
    eps = (U32 * (lg - lg.amax(-1, keepdim=True)).abs()).amax(-1, keepdim=True)
    e_aw = aw * (torch.expm1(2.0 * eps) + 16.0 * U32) * SECOND + TINY
    zero = torch.zeros_like(off[..., 0])
    y_div = float(W if plant == "offset_y_over_W" else H)     # what the y offset is divided by
    loc_x, dpx, raw_x = _position(rx, off[..., 0], zero, float(W), float(H))
    loc_y, dpy, raw_y = _position(ry, off[..., 1], zero, float(H), y_div)
    assert float(dpx.max()) < 0.5 and float(dpy.max()) < 0.5
    px, py = loc_x * W - 0.5, loc_y * H - 0.5
    inside = lambda r: (r >= 0.0) & (r <= 1.0)  # noqa: E731
    mask_x, mask_y = inside(raw_x), inside(raw_y)
    if plant == "clamp_mask_exclusive":
        on_edge = (raw_x == 0.0) | (raw_x == 1.0) | (raw_y == 0.0) | (raw_y == 1.0)
        if not bool(on_edge.any()):
            raise NotExercised("no location exactly on 0 or 1")
        mask_x, mask_y = (raw_x > 0.0) & (raw_x < 1.0), (raw_y > 0.0) & (raw_y < 1.0)
    if plant == "clamp_mask_ignored":
        if bool((mask_x & mask_y).all()):
            raise NotExercised("no point is clamped")
        mask_x, mask_y = torch.ones_like(mask_x), torch.ones_like(mask_y)
    x0f, y0f = torch.floor(px), torch.floor(py)
    x0, y0 = x0f.long(), y0f.long()
    wx1, wy1 = px - x0f, py - y0f
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    # the gather: d_ol
    v = ins["value"].double().reshape(B, H, W, NH, CH)
    shape = (B, T, NH, NP)
    b_idx = torch.arange(B).view(B, 1, 1, 1).expand(shape)
    h_idx = torch.arange(NH).view(1, 1, NH, 1).expand(shape)
    t_idx = tok.view(1, T, 1, 1).expand(shape)
    d, a = _cell(v, g, b_idx, h_idx, y0, x0, H, W)
    G, PX, PY = _blend(d, wx0, wx1, wy0, wy1)
    if plant == "border_padding_in_derivative":
        if not bool(((px < 0) | (px > W - 1) | (py < 0) | (py > H - 1)).any()):
            raise NotExercised("no footprint leaves the image")
        _, PX, PY = _blend(_cell(v, g, b_idx, h_idx, y0, x0, H, W, border=True)[0], wx0, wx1, wy0, wy1)
    if plant == "left_derivative_at_kink":
        kx, ky = (px == x0f) & (dpx > 0), (py == y0f) & (dpy > 0)
        if not bool((kx | ky).any()):
            raise NotExercised("no position exactly on a kink")
        _, PXl, _ = _blend(_cell(v, g, b_idx, h_idx, y0, x0 - 1, H, W)[0], wx0, wx1, wy0, wy1)
        _, _, PYl = _blend(_cell(v, g, b_idx, h_idx, y0 - 1, x0, H, W)[0], wx0, wx1, wy0, wy1)
        PX, PY = torch.where(kx, PXl, PX), torch.where(ky, PYl, PY)
    s = (aw * G).sum(-1, keepdim=True)
    dlogit = aw * (G if plant == "dlogit_without_mean_term" else G - s)
    fx = 1.0 if plant == "doffx_without_W_over_H" else rWH
    fy = rWH if plant == "doffy_times_W_over_H" else 1.0
    doffx = torch.where(mask_x, aw * PX * fx, zero)
    doffy = torch.where(mask_y, aw * PY * fy, zero)
    d_ol = torch.cat([torch.stack([doffx, doffy], -1).reshape(B, T, 128), dlogit.reshape(B, T, 64)], -1)
    if plant == "odd_tail_takes_previous_token":
        if (B * N) % 2 == 0 or B * N == 1 or tokens is not None:
            raise NotExercised("no odd tail besides token 0's")
        d_ol = d_ol.reshape(B * N, 192).clone()
        d_ol[-1] = d_ol[-2]
        d_ol = d_ol.reshape(B, N, 192)

    bound_ol = widened = None
    if bounds:
        lo_x, hi_x, lo_y, hi_y = torch.floor(px - dpx), torch.floor(px + dpx), torch.floor(py - dpy), torch.floor(py + dpy)
        xw, yw = lo_x != hi_x, lo_y != hi_y
        x_alt = torch.where(lo_x < x0f, x0 - 1, x0 + 1)
        y_alt = torch.where(lo_y < y0f, y0 - 1, y0 + 1)
        mx = _cell_maxima(d, a)
        side_x, side_y = torch.zeros_like(PX), torch.zeros_like(PY)
        g_pt = g.expand(B, T, NH, NP, CH)
        for sel, xs, ys, which in ((xw, x_alt, y0, "x"), (yw, x0, y_alt, "y"), (xw & yw, x_alt, y_alt, "xy")):
            if not bool(sel.any()):
                continue
            ds_, as_ = _cell(v, g_pt[sel], b_idx[sel], h_idx[sel], ys[sel], xs[sel], H, W)
            for m, other in zip(mx, _cell_maxima(ds_, as_)):
                m[sel] = torch.maximum(m[sel], other)
            _, PXo, PYo = _blend(ds_, wx0[sel], wx1[sel], wy0[sel], wy1[sel])
            if which == "x":
                side_x[sel] = (PXo - PX[sel]).abs()
            if which == "y":
                side_y[sel] = (PYo - PY[sel]).abs()
        SGx, SGy, X, MG, MPX, MPY = mx
        ru = DOT_ROUNDINGS * U32
        dG = (SGx * dpx + SGy * dpy + ru * MG) * SECOND
        dPX = side_x + (X * dpy + ru * MPX) * SECOND
        dPY = side_y + (X * dpx + ru * MPY) * SECOND
        unsure = lambda raw, o: (raw.abs() <= _E_l(raw, o, float(H))) | ((raw - 1.0).abs() <= _E_l(raw, o, float(H)))  # noqa: E731
        ux, uy = unsure(raw_x, off[..., 0]), unsure(raw_y, off[..., 1])

        def e_off(Pd, dP, f, mask, un):
            e = f * ((e_aw + 3.0 * U32 * aw) * (Pd.abs() + dP) + aw * dP) * SECOND + 4.0 * max(1.0, f) * TINY
            e = torch.where(un, e + (f * aw * Pd).abs(), e)
            return torch.where(mask | un, e, torch.zeros_like(e))

        E_x, E_y = e_off(PX, dPX, rWH, mask_x, ux), e_off(PY, dPY, 1.0, mask_y, uy)
        Gup = G.abs() + dG
        ds = ((e_aw * Gup + aw * dG).sum(-1, keepdim=True) + 5.0 * U32 * ((aw + e_aw) * Gup).sum(-1, keepdim=True)) * SECOND
        E_lg = ((e_aw + 2.0 * U32 * aw) * ((G - s).abs() + dG + ds) + aw * (dG + ds)) * SECOND + TINY
        bound_ol = torch.cat([torch.stack([E_x, E_y], -1).reshape(B, T, 128), E_lg.reshape(B, T, 64)], -1)
        widened = float((xw | yw | ux | uy).double().mean())

    # the scatter: d_value
    HW_NH = N * NH
    d_value = torch.zeros(B * HW_NH, CH, dtype=torch.float64)
    E_v = torch.zeros(B * HW_NH, CH, dtype=torch.float64) if bounds else None
    n_adds = torch.zeros(B * HW_NH, dtype=torch.float64)
    e_s = fx_exponents(d_out)
    F_ = fx_bits(N)
    step = torch.tensor([2.0 ** (e - F_) for e in e_s], dtype=torch.float64)
    if plant == "scale_from_whole_batch":
        if len(set(e_s)) == 1:
            raise NotExercised("every sample has the same scale")
        step_b = torch.full_like(step, float(step.max())).view(B, 1, 1, 1).expand(shape)
    tile_x, tile_y = (t_idx % W) // TS * TS - RAD, (t_idx // W) // TS * TS - RAD
    n_far = 0
    g_pt = g.expand(B, T, NH, NP, CH)
    for dy in ((-1, 0, 1, 2) if bounds else (0, 1)):
        for dx in ((-1, 0, 1, 2) if bounds else (0, 1)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            hx, hy = (1.0 - (px - xi).abs()).clamp_min(0.0), (1.0 - (py - yi).abs()).clamp_min(0.0)
            cell = yi * (H if plant == "dvalue_cell_index_H_W_swapped" else W) + xi
            if plant == "dvalue_cell_index_H_W_swapped":
                cell = cell % N
            idx = (b_idx * N + cell) * NH + h_idx
            far = ok & ~((xi - tile_x >= 0) & (xi - tile_x < TS + 2 * RAD) & (yi - tile_y >= 0) & (yi - tile_y < TS + 2 * RAD))
            if dx in (0, 1) and dy in (0, 1):
                sel = ok & (hx * hy > 0)
                n_far += int((far & sel).sum())
                if plant == "dvalue_far_taps_dropped":
                    sel = sel & ~far
                src = (aw * hx * hy)[sel][:, None] * g_pt[sel]
                if plant == "scale_from_whole_batch":
                    st = step_b[sel][:, None]
                    src = torch.round(src / st) * st
                d_value.index_add_(0, idx[sel], src)
            if bounds:
                Hx = (1.0 - ((px - xi).abs() - dpx).clamp_min(0.0)).clamp_min(0.0)
                Hy_ = (1.0 - ((py - yi).abs() - dpy).clamp_min(0.0)).clamp_min(0.0)
                sel = ok & (Hx * Hy_ > 0)
                if not bool(sel.any()):
                    continue
                tx, ty = torch.where(Hx > 0, dpx, zero), torch.where(Hy_ > 0, dpy, zero)
                A = (aw * (tx * Hy_ + hx * ty) + (e_aw + 4.0 * U32 * aw + TINY) * Hx * Hy_) * SECOND
                E_v.index_add_(0, idx[sel], A[sel][:, None] * g_pt[sel].abs())
                n_adds.index_add_(0, idx[sel], torch.ones(int(sel.sum()), dtype=torch.float64))
    if plant == "dvalue_far_taps_dropped" and n_far == 0:
        raise NotExercised("no tap leaves its token tile's window")
    d_value = d_value.reshape(B, N, C)
    bound_value = None
    if bounds:
        half = (0.5 * step).view(B, 1, 1)
        E_v = E_v.reshape(B, N, C) + (n_adds.reshape(B, N, NH, 1) * half[..., None]).expand(B, N, NH, CH).reshape(B, N, C)
        bound_value = E_v + U32 * (d_value.abs() + E_v) * SECOND + TINY
    return Grad(d_value, d_ol, bound_value, bound_ol, widened, aw, px, py, raw_x, raw_y, mask_x, mask_y, n_far,
                n_adds.reshape(B, N, NH))


def split_ol(t):
    """(offsets part, logits part) of a d_ol-shaped tensor."""
    return t[..., :128], t[..., 128:]


def error_over_bound(got, ref, bound):
    """max |got - ref| / bound; an element whose bound is 0 (a surely masked offset gradient) counts 0 when it is exact."""
    d = (got.detach().double().cpu() - ref).abs()
    return float(torch.where((bound == 0) & (d == 0), torch.zeros_like(d), d / bound).max())


# ----------------------------------------------------------------------------------------------------------------------
# float32 / int64 emulation of the three kernels, operation by operation
# ----------------------------------------------------------------------------------------------------------------------
def emulate_f32(case, ins, contract, d_out=None):
    """deform_grad_ol_kernel, deform_absmax_kernel and deform_scatter_kernel + deform_convert_kernel of
    csrc/deform_grad.hip in float32 torch arithmetic (the fixed-point scatter as an int64 index_add_).  contract: the px
    statement and the inner pairs of dot8 as FMAs.  Returns (d_value (B,N,256), d_ol (B,N,192)), fp32."""
    B, H, W = case.B, case.H, case.W
    N = H * W
    one = torch.tensor(1.0, dtype=torch.float32)
    d_out = ins["d_out"] if d_out is None else d_out
    ol = ins["ol"].reshape(B, N, 192)
    assert ol.dtype == torch.float32 and d_out.dtype == torch.float32
    off = ol[..., :128].reshape(B, N, NH, NP, 2)
    lg = ol[..., 128:].reshape(B, N, NH, NP)
    e = torch.exp(lg - lg.amax(-1, keepdim=True))
    pair = e[..., 0::2] + e[..., 1::2]
    s2 = pair[..., 0::2] + pair[..., 1::2]
    aw = e / (s2[..., 0] + s2[..., 1])[..., None]
    pts = ins["ref_pts"].expand(B, N, 2)
    fH, fW = torch.tensor(float(H)), torch.tensor(float(W))

    def axis(r, o, n):
        l = r + o / fH
        m = ((l >= 0.0) & (l <= 1.0)).float()
        l = l.clamp(0.0, 1.0)
        t = (l * 2.0 - 1.0) + 1.0
        p = (_fma32(t, n.expand_as(t), -one.expand_as(t)) if contract else t * n - 1.0) / 2.0
        p0 = torch.floor(p)
        return p0.long(), p - p0, (p0 + 1.0) - p, m

    x0, wx1, wx0, mx = axis(pts[..., 0].reshape(B, N, 1, 1), off[..., 0], fW)
    y0, wy1, wy0, my = axis(pts[..., 1].reshape(B, N, 1, 1), off[..., 1], fH)
    shape = (B, N, NH, NP)
    b_idx = torch.arange(B).view(B, 1, 1, 1).expand(shape)
    h_idx = torch.arange(NH).view(1, 1, NH, 1).expand(shape)
    v = ins["value"].float().reshape(B, H, W, NH, 4, 8)                    # a lane's 8 channels
    g = d_out.reshape(B, N, NH, 1, 4, 8)

    def dot(dy, dx):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        rows = v[b_idx, yi.clamp(0, H - 1), xi.clamp(0, W - 1), h_idx]      # (B,N,NH,NP,4,8)
        prod = rows * g
        if contract:
            pr = _fma32(rows[..., 0::2], g[..., 0::2].expand_as(rows[..., 0::2]), prod[..., 1::2])
        else:
            pr = prod[..., 0::2] + prod[..., 1::2]
        q = pr[..., 0::2] + pr[..., 1::2]
        return torch.where(ok[..., None], q[..., 0] + q[..., 1], torch.zeros(()))     # (B,N,NH,NP,4)

    quad = lambda t: (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])  # noqa: E731
    L = lambda w: w[..., None]  # noqa: E731
    d00, d01, d10, d11 = dot(0, 0), dot(0, 1), dot(1, 0), dot(1, 1)
    G = quad(L(wy0) * (L(wx0) * d00 + L(wx1) * d01) + L(wy1) * (L(wx0) * d10 + L(wx1) * d11))
    PX = quad(L(wy0) * (d01 - d00) + L(wy1) * (d11 - d10))
    PY = quad(L(wx0) * (d10 - d00) + L(wx1) * (d11 - d01))
    awG = aw * G
    s = quad(awG[..., 0::2] + awG[..., 1::2])[..., None]
    rWH = fW / fH
    doff = torch.stack([mx * (aw * PX) * rWH, my * (aw * PY)], -1)
    d_ol = torch.cat([doff.reshape(B, N, 128), (aw * (G - s)).reshape(B, N, 64)], -1)
    assert d_ol.dtype == torch.float32

    F_ = fx_bits(N)
    shift = torch.tensor([float(F_ - e_) for e_ in fx_exponents(d_out)], dtype=torch.float64)
    scale = (2.0 ** shift).view(B, 1, 1, 1)
    sums = torch.zeros(B * N * NH, CH, dtype=torch.int64)
    gd = d_out.double().reshape(B, N, NH, 1, CH).expand(B, N, NH, NP, CH)
    for dy, dx, wy, wx in ((0, 0, wy0, wx0), (0, 1, wy0, wx1), (1, 0, wy1, wx0), (1, 1, wy1, wx1)):
        xi, yi = x0 + dx, y0 + dy
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        wd = ((wx * wy * aw).double() * scale)[ok]
        add = torch.round(gd[ok] * wd[:, None])                            # exact product, one round-half-even
        assert float(add.abs().max()) < 2.0 ** 51 if add.numel() else True
        sums.index_add_(0, ((b_idx * N + yi * W + xi) * NH + h_idx)[ok], add.long())
    d_value = (sums.reshape(B, N * C).double() * (2.0 ** -shift).view(B, 1)).float().reshape(B, N, C)
    return d_value, d_ol
